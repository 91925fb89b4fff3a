// Reading .pcd files on the device (csrc/pcd_read.hip): the header parsed on the host, an ASCII body cut into point lines and parsed
// into records of an lsr_pc2_layout in HBM (csrc/pcd_parse.hpp is the per-token arithmetic), a binary body gathered, a compressed body
// inflated (csrc/pcd_lzf.hip), and what a handle
// keeps for it (lsr_decode_pcd, lsr_load_pcd, lsr_set_input_target_pcd; the entries themselves are csrc/pcd_input.hip).
#pragma once
#include "common.hpp"
#include "pcd_parse.hpp"

namespace lsr {

constexpr int PCDR_WG = 256;          // threads per workgroup of the line, index and parse passes
constexpr int PCDR_RUN = 64;          // body bytes per thread of the line and index passes: four 16-byte loads
constexpr int PCDR_MAX_LINE = 1024;
constexpr int PCDR_PIECE_MIN = 2048, PCDR_PIECE_MAX = 1 << 28, PCDR_PIECE_DEFAULT = 1 << 26;
static_assert(PCDR_MAX_LINE == LSR_PCD_READ_MAX_LINE_BYTES, "header and core disagree");

// the header of a file, with what the passes need besides lsr_pcd_info
struct PcdHeader {
  lsr_pcd_info info;
  int tok[4];      // ASCII: the index, among a line's tokens, of x y z intensity (-1: no intensity)
  int src[4];      // binary: their byte offsets inside a record (-1: no intensity)
  int n_tokens;    // ASCII: tokens a line must have
};
// Parses the head of a file image.  LSR_OK, or the status lsr_parse_pcd_header documents with the reason in lsr_last_error();
// *incomplete (nullable): the bytes ended before the DATA line did — more of the file may help.  H->info is filled before either
// LSR_ERR_NOT_IMPLEMENTED is returned.  take_compressed: DATA binary_compressed is no error (LSR_PCD_READ_COMPRESSED).
int pcd_parse_header(const void* bytes, size_t n_bytes, PcdHeader* H, bool* incomplete = nullptr, bool take_compressed = false);

struct PcdOutFields {   // where the four values go in a record of the output layout; off[3] < 0: the intensity is dropped
  int step;
  int off[4];
};
struct PcdAsciiPlan {
  int tok[4];
  int n_tokens;
  PcdOutFields out;
};
struct PcdBinaryPlan {
  unsigned int rec_bytes;
  int src[4];
  PcdOutFields out;
};

// a record of the output layout from the four values' bits: every byte outside the fields zero (binary, compressed and ASCII bodies alike)
__device__ inline void pcdr_store_record(unsigned char* rec, const PcdOutFields& O, bool wide, const uint32_t* v) {
  if (wide) {
    uint4* q = reinterpret_cast<uint4*>(rec);
    q[0] = make_uint4(v[0], v[1], v[2], 0u);
    q[1] = make_uint4(v[3], 0u, 0u, 0u);
    return;
  }
  uint32_t* w = reinterpret_cast<uint32_t*>(rec);   // records and offsets are 4-byte aligned (checked by the entry points)
  const int nw = O.step >> 2;
  for (int j = 0; j < nw; j++) {
    uint32_t x = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (O.off[k] == 4 * j) x = v[k];
    w[j] = x;
  }
}

__device__ inline bool pcdr_is_wide(const PcdOutFields& O, const unsigned char* records) {
  return O.step == 32 && O.off[0] == 0 && O.off[1] == 4 && O.off[2] == 8 && O.off[3] == 16 && ((uintptr_t)records & 15u) == 0;
}

// the first bad line of a parse pass and the tokens it left to the host
enum PcdLineError : unsigned int { PCDR_ERR_TOO_LONG = 1, PCDR_ERR_SHORT = 2, PCDR_ERR_TOKEN = 3 };
struct PcdReadStatus {
  unsigned long long first_error;   // (offset of the line's first byte inside the text << 3) | PcdLineError; ~0: none
  unsigned int unresolved;          // tokens left unresolved so far
  unsigned int pad;
};
constexpr unsigned long long PCDR_NO_ERROR = ~0ull;

// ---- DATA binary_compressed (csrc/pcd_lzf.hip) ----
constexpr int LZF_BLOCK = 4096;       // stream bytes per workgroup of the map and source passes, staged in LDS
constexpr int LZF_ENTRIES = 33;       // a token has at most 33 bytes: a block is entered at its bytes 0 .. 32
constexpr int LZF_MAX_PASSES = 32;    // pointer-doubling launches: 31 would do for 2^31 - 1 bytes one hop at a time, 14 with four hops a launch
constexpr unsigned int LZF_LITERAL = 0x80000000u;   // source word: this bit | stream byte index; without it: an earlier output byte
enum PcdLzfError : unsigned int { LZF_ERR_CUT = 1, LZF_ERR_TOO_LONG = 2, LZF_ERR_BEFORE_START = 3 };
struct PcdLzfInfo {
  unsigned long long first_error;     // (offset of the token's control byte inside the stream << 3) | PcdLzfError; ~0: none
  unsigned long long total_out;       // bytes the whole stream inflates to
  unsigned int unresolved[LZF_MAX_PASSES];   // per doubling pass: some source word still points at an output byte
};

struct PcdReadState {
  int piece_bytes = PCDR_PIECE_DEFAULT;   // LSR_PCD_READ_PIECE_BYTES
  int read_compressed = 0;                // LSR_PCD_READ_COMPRESSED
  double parse_ms = 0.0;                  // LSR_PCD_PARSE_MS
  double inflate_ms = 0.0;                // LSR_PCD_INFLATE_MS
  int unresolved = 0;                     // LSR_PCD_UNRESOLVED_TOKENS
  DevBuf<unsigned char> text;             // the piece (or the body of a host image) being parsed
  DevBuf<PcdRun> wg_runs;                 // line pass: what each workgroup's bytes do
  DevBuf<unsigned long long> first_slot;  // scan: the number of point lines in front of each workgroup, the total behind them
  DevBuf<unsigned char> entry_state;      // scan: the state each workgroup is entered in
  DevBuf<unsigned int> line_start;        // index pass: the offset of every point line's first byte inside the text
  DevBuf<unsigned char> records;          // every record of the file in the output layout; copied out only when the whole file was good
  DevBuf<unsigned char> flags;            // per record: bit k = token k (x y z intensity) is left to the host
  DevBuf<PcdReadStatus> status;
  PinBuf<PcdReadStatus> h_status;
  PinBuf<unsigned long long> h_total;
  PinBuf<unsigned char> pin[2];           // lsr_load_pcd: piece k + 1 is read into one while piece k is parsed from the other
  DevBuf<unsigned char> target;           // lsr_set_input_target_pcd: the file's records {32; 0,4,8,16}
  // DATA binary_compressed: per block and entry where the walk leaves into the next block and how many bytes it puts out; per block
  // its true entry and first output byte (the last entry: the total); per output byte its source word
  DevBuf<unsigned char> lzf_exit, lzf_entry;
  DevBuf<unsigned int> lzf_outc, lzf_src;
  DevBuf<unsigned long long> lzf_out_start;
  DevBuf<PcdLzfInfo> lzf_info;
  PinBuf<PcdLzfInfo> h_lzf_info;
  enum { EV_L0 = 0, EV_L1, EV_P0, EV_P1, EV_I0, EV_I1, EV_COUNT };
  hipEvent_t ev[EV_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool have_events = false;
  PcdReadState() = default;
  PcdReadState(const PcdReadState&) = delete;
  PcdReadState& operator=(const PcdReadState&) = delete;
  ~PcdReadState() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int ensure_events() {
    if (have_events) return LSR_OK;
    for (hipEvent_t& e : ev)
      if (!e) LSR_HIP(hipEventCreate(&e));
    have_events = true;
    return LSR_OK;
  }
};

// workgroups of the line and index passes over a text of n bytes at d_text
inline size_t pcdr_blocks(const unsigned char* d_text, size_t n) {
  return (pcd_run_count(d_text, n, PCDR_RUN) + PCDR_WG - 1) / PCDR_WG;
}

// Line pass and scan of a text (any alignment, 0 < n < 2^32) on `stream`: d_wg_runs[pcdr_blocks], d_entry_state[pcdr_blocks],
// d_first_slot[pcdr_blocks + 1] (the last entry: the number of point lines in the text).  The text is entered in state 0.
int pcd_read_lines(const unsigned char* d_text, size_t n, PcdRun* d_wg_runs, unsigned long long* d_first_slot, unsigned char* d_entry_state,
                   hipStream_t stream);
// Index pass: d_line_start[k] = offset of point line k's first byte, for k < n_keep.  One writer per slot.
int pcd_read_index(const unsigned char* d_text, size_t n, const unsigned long long* d_first_slot, const unsigned char* d_entry_state,
                   size_t n_keep, unsigned int* d_line_start, hipStream_t stream);
// Parse pass: one point line per thread; record k of d_records (4-byte aligned) and d_flags[k] written for every good line k < n_lines.
int pcd_read_parse(const unsigned char* d_text, size_t n, const unsigned int* d_line_start, size_t n_lines, const PcdAsciiPlan& plan,
                   unsigned char* d_records, unsigned char* d_flags, PcdReadStatus* d_status, hipStream_t stream);
// Binary body: n_records records of plan.rec_bytes at d_body (any alignment), the four fields copied bit for bit.
int pcd_read_binary(const unsigned char* d_body, size_t n_records, const PcdBinaryPlan& plan, unsigned char* d_records, hipStream_t stream);
// DATA binary_compressed: the LZF stream of n_stream bytes at d_stream (any alignment; 0 < n_stream, n_out < 2^31) inflated — never
// as an image: every output byte gets the index of the stream byte it is a copy of — and the n_records records gathered from it
// (field-major image: field k's block starts at n_records * plan.src[k]) into d_records.  Waits for the stream (the doubling passes
// are counted on the host).  A bad stream is LSR_ERR_INVALID_ARGUMENT, the token named by file_offset (of the stream's first byte) +
// its offset; nothing is written to d_records then.  ms (nullable): the hipEvent time of the launches is added (S.ev[EV_I0 / EV_I1]).
int pcd_lzf_inflate(PcdReadState& S, const unsigned char* d_stream, size_t n_stream, size_t n_out, size_t n_records, const PcdBinaryPlan& plan,
                    unsigned char* d_records, unsigned long long file_offset, double* ms, hipStream_t stream);

}  // namespace lsr
