// map.pcd from the device (csrc/pcd_text.hip): records of an lsr_pc2_layout in HBM -> the text pcl::io::savePCDFileASCII writes for
// them, and what a handle keeps for it (lsr_format_pcd_ascii, lsr_save_pcd_ascii, lsr_save_map_pcd_ascii).
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int PCD_WG = 256;                 // records per workgroup, one per thread
constexpr int PCD_MAX_LINE_BYTES = 60;      // four fields of 14 bytes, three blanks, the newline
constexpr int PCD_MAX_HEADER_BYTES = 256;
constexpr int PCD_PIECE_MIN = 64, PCD_PIECE_MAX = 1 << 22, PCD_PIECE_DEFAULT = 1 << 20;
static_assert(PCD_MAX_LINE_BYTES == LSR_PCD_ASCII_MAX_LINE_BYTES && PCD_MAX_HEADER_BYTES == LSR_PCD_ASCII_MAX_HEADER_BYTES, "header and core disagree");

struct PcdFields {   // byte offsets of the fields of a line, in line order (x y z [intensity])
  int step, n_fields;
  int off[4];
};

struct PcdState {
  int piece_records = PCD_PIECE_DEFAULT;   // LSR_PCD_PIECE_RECORDS
  double format_ms = 0.0;                  // LSR_PCD_FORMAT_MS
  // per piece in flight (two): workgroup sums of the line lengths, their exclusive scan (+ the total behind it)
  DevBuf<unsigned int> block_sums[2];
  DevBuf<unsigned long long> offsets[2];
  DevBuf<unsigned char> text;              // the text of one piece (or of a whole image) on its way to the host
  PinBuf<unsigned char> pin[2];            // lsr_save_pcd_ascii: piece k + 1 lands in one while the caller's thread writes piece k from the other
  PinBuf<unsigned long long> totals;       // [2]: a piece's byte count, read back before its text is laid out
  PinBuf<unsigned char> header;
  DevBuf<unsigned char> map;               // lsr_save_map_pcd_ascii: the assembled map, XYZI records
  // per piece in flight: length launches begin / end, length known, write launch begin / end, text in pinned memory
  enum { EV_L0 = 0, EV_L1, EV_LEN, EV_W0, EV_W1, EV_DONE, EV_PER_PIECE };
  hipEvent_t ev[2][EV_PER_PIECE] = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
  bool have_events = false;
  PcdState() = default;
  PcdState(const PcdState&) = delete;
  PcdState& operator=(const PcdState&) = delete;
  ~PcdState() {
    for (auto& row : ev)
      for (hipEvent_t e : row)
        if (e) (void)hipEventDestroy(e);
  }
  int ensure_events() {
    if (have_events) return LSR_OK;
    for (auto& row : ev)
      for (hipEvent_t& e : row)
        if (!e) LSR_HIP(hipEventCreate(&e));
    have_events = true;
    return LSR_OK;
  }
};

// the PCD header of a cloud of n records built by `+=` (width n, height 1, default viewpoint), its last line "DATA <data_word>"; returns
// its length (< PCD_MAX_HEADER_BYTES)
int pcd_header_text(size_t n, bool with_intensity, char* out /* PCD_MAX_HEADER_BYTES */, const char* data_word = "ascii");

inline size_t pcd_blocks(size_t n) { return (n + PCD_WG - 1) / PCD_WG; }

// Length pass and scan of n records (n <= INT32_MAX) on `stream`: d_block_sums[pcd_blocks(n)] the bytes of each workgroup's lines,
// d_offsets[pcd_blocks(n) + 1] their exclusive scan with the total in the last entry.
int pcd_text_lengths(const void* d_records, size_t n, const PcdFields& F, unsigned int* d_block_sums, unsigned long long* d_offsets,
                     hipStream_t stream);
// Write pass: the lines of the n records, back to back, at d_text (any alignment; d_offsets' last entry bytes).  One writer per byte.
int pcd_text_write(const void* d_records, size_t n, const PcdFields& F, const unsigned long long* d_offsets, unsigned char* d_text,
                   hipStream_t stream);

}  // namespace lsr
