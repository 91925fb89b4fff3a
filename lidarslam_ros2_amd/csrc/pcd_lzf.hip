// DATA binary_compressed: one LZF stream (liblzf's lzf_decompress, restated in include/lidarslam_reg.h) inflated on the device, with no
// host pass over the stream.  LZF is parallel for three reasons: where a token ends depends on its control byte alone; a token has at
// most 33 bytes, so a block of the stream can only be entered at its bytes 0 .. 32; and a back reference "output byte k is output byte
// k - distance" is a pointer that resolves by doubling.  The inflated image itself never exists: every output byte gets a 32-bit SOURCE
// word — LZF_LITERAL | index of the stream byte it is a copy of, or the index of an earlier output byte — and the records are gathered
// from the stream through the resolved words.
//   lzf_map_kernel      a workgroup (one wave) per LZF_BLOCK stream bytes, staged in LDS: lane e < 33 walks the block's tokens from
//                       byte e and records where it leaves into the next block and how many bytes it puts out (step a and b in one walk)
//   lzf_scan_kernel     ONE workgroup: the blocks' 33-entry maps composed in order (each thread composes a chunk, thread 0 the chunks),
//                       the stream entered at byte 0 -> per block its true entry and its first output byte (64 bits), the total
//   lzf_source_kernel   a workgroup per block: thread 0 walks the tokens from the true entry into an LDS table (stream position, output
//                       offset) and reports the bad ones; then every thread takes output bytes of the block in turn, finds its token by
//                       bisection and stores the source word — one writer per word, coalesced
//   lzf_double_kernel   src[k] = src[src[k]], four hops a launch, for the words that still point at output; a word read while another
//                       thread replaces it is the old or the new one, both ancestors of k: the result is fixed whatever the scheduling.
//                       The host launches it until a pass leaves nothing unresolved: a launch multiplies what a word spans by at
//                       least 5 (its own hop and four more), so a run as long as the largest file (depth 2^31) takes 14 launches
//   lzf_records_kernel  one point per thread: the 4 bytes of x y z [intensity] fetched from the stream through their source words, the
//                       record of the output layout stored whole, as pcdr_binary_kernel does
// Errors: a token cut by the end of the stream, output past uncompressed_size, a reference before the first output byte — the earliest
// in stream order wins (a minimum over the control byte's offset, the only atomic here); a stream that ends short shows in the total.
// No store depends on the stream being good: a source word is only written for k < n_out and always names a stream byte < n_stream or
// an output byte < k.
#include "pcd_read.hpp"

namespace lsr {

namespace {

constexpr int LZF_STAGE = LZF_BLOCK + 8;      // a token starting at the block's last byte has its length byte and distance byte behind it
constexpr int LZF_SOURCE_WG = 256;
constexpr int LZF_SCAN_WG = 1024;
constexpr int LZF_MAX_TOKENS = LZF_BLOCK / 2 + 1;   // the shortest token has two bytes
constexpr int LZF_HOPS = 4;

// the block's bytes (those inside the stream) into LDS
__device__ inline void lzf_stage(const unsigned char* __restrict__ in, size_t base, size_t n, unsigned char* lds, int tid, int wg) {
  const size_t room = n - base;
  const int len = (int)(room < (size_t)LZF_STAGE ? room : (size_t)LZF_STAGE);
  for (int i = tid; i < len; i += wg) lds[i] = in[base + i];
}

// the token whose control byte is block byte pos: its length in the stream and in the output.  A byte behind the stream reads as 0
// (such a token is cut: an error wherever it matters).
__device__ inline void lzf_token(const unsigned char* lds, int pos, size_t base, size_t n, int* t_len, int* o_len) {
  const unsigned int c = lds[pos];
  if (c < 32u) { *t_len = (int)c + 2; *o_len = (int)c + 1; return; }
  const unsigned int len = c >> 5;
  if (len == 7u) {
    const unsigned int ext = base + (size_t)pos + 1 < n ? lds[pos + 1] : 0u;
    *t_len = 3; *o_len = 9 + (int)ext;
  } else {
    *t_len = 2; *o_len = (int)len + 2;
  }
}

__global__ __launch_bounds__(64) void lzf_map_kernel(const unsigned char* __restrict__ in, size_t n, unsigned char* __restrict__ exit_map,
                                                     unsigned int* __restrict__ out_count) {
  __shared__ unsigned char lds[LZF_STAGE];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * LZF_BLOCK;
  lzf_stage(in, base, n, lds, tid, 64);
  __syncthreads();
  if (tid >= LZF_ENTRIES) return;
  const int L = (int)(n - base < (size_t)LZF_BLOCK ? n - base : (size_t)LZF_BLOCK);
  int pos = tid;
  unsigned int out = 0;
  while (pos < L) {
    int t_len, o_len;
    lzf_token(lds, pos, base, n, &t_len, &o_len);
    pos += t_len;
    out += (unsigned int)o_len;
  }
  // pos - L <= 32: the last token began inside the block (or pos is the entry itself, in a last block shorter than the entry)
  exit_map[(size_t)blockIdx.x * LZF_ENTRIES + tid] = (unsigned char)(pos - L);
  out_count[(size_t)blockIdx.x * LZF_ENTRIES + tid] = out;
}

__global__ __launch_bounds__(LZF_SCAN_WG) void lzf_scan_kernel(const unsigned char* __restrict__ exit_map, const unsigned int* __restrict__ out_count,
                                                               long long nb, unsigned char* __restrict__ entry,
                                                               unsigned long long* __restrict__ out_start, PcdLzfInfo* __restrict__ info) {
  __shared__ unsigned char m[LZF_ENTRIES][LZF_SCAN_WG];   // what each thread's chunk of blocks does to an entry
  __shared__ unsigned char chunk_entry[LZF_SCAN_WG];
  __shared__ unsigned long long chunk_first[LZF_SCAN_WG];
  const int tid = threadIdx.x;
  const long long chunk = (nb + LZF_SCAN_WG - 1) / LZF_SCAN_WG;
  const long long lo = min((long long)tid * chunk, nb), hi = min(lo + chunk, nb);
  for (int e = 0; e < LZF_ENTRIES; e++) m[e][tid] = (unsigned char)e;
  for (long long j = lo; j < hi; j++) {
    const unsigned char* row = exit_map + j * LZF_ENTRIES;
    for (int e = 0; e < LZF_ENTRIES; e++) m[e][tid] = row[m[e][tid]];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned int e = 0;   // the stream is entered at its first byte
    for (int t = 0; t < LZF_SCAN_WG; t++) {
      chunk_entry[t] = (unsigned char)e;
      e = m[e][t];
    }
  }
  __syncthreads();
  unsigned int e = chunk_entry[tid];
  unsigned long long sum = 0;
  for (long long j = lo; j < hi; j++) {
    entry[j] = (unsigned char)e;
    out_start[j] = sum;
    sum += out_count[j * LZF_ENTRIES + e];
    e = exit_map[j * LZF_ENTRIES + e];
  }
  chunk_first[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < LZF_SCAN_WG; t++) {
      const unsigned long long s = chunk_first[t];
      chunk_first[t] = run;
      run += s;
    }
    out_start[nb] = run;
    info->total_out = run;
  }
  __syncthreads();
  const unsigned long long first = chunk_first[tid];
  for (long long j = lo; j < hi; j++) out_start[j] += first;
}

__global__ __launch_bounds__(LZF_SOURCE_WG) void lzf_source_kernel(const unsigned char* __restrict__ in, size_t n, unsigned long long n_out,
                                                                   const unsigned char* __restrict__ entry,
                                                                   const unsigned long long* __restrict__ out_start,
                                                                   unsigned int* __restrict__ src, PcdLzfInfo* __restrict__ info) {
  __shared__ unsigned char lds[LZF_STAGE];
  __shared__ unsigned short tok_pos[LZF_MAX_TOKENS];
  __shared__ unsigned int tok_out[LZF_MAX_TOKENS + 1];   // relative to the block's first output byte; the last entry: the block's output
  __shared__ int n_tok;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * LZF_BLOCK;
  const unsigned long long o0 = out_start[blockIdx.x];
  lzf_stage(in, base, n, lds, tid, LZF_SOURCE_WG);
  __syncthreads();
  if (tid == 0) {
    const int L = (int)(n - base < (size_t)LZF_BLOCK ? n - base : (size_t)LZF_BLOCK);
    int pos = entry[blockIdx.x], t = 0;
    unsigned int o = 0;
    while (pos < L) {
      int t_len, o_len;
      lzf_token(lds, pos, base, n, &t_len, &o_len);
      tok_pos[t] = (unsigned short)pos;
      tok_out[t] = o;
      const unsigned int c = lds[pos];
      unsigned int err = 0;
      if (base + (size_t)pos + (size_t)t_len > n) {
        err = LZF_ERR_CUT;
      } else if (o0 + o + (unsigned int)o_len > n_out) {
        err = LZF_ERR_TOO_LONG;
      } else if (c >= 32u) {
        const unsigned int dist = (((c & 31u) << 8) | lds[pos + t_len - 1]) + 1u;
        if ((unsigned long long)dist > o0 + o) err = LZF_ERR_BEFORE_START;
      }
      if (err) atomicMin(&info->first_error, ((unsigned long long)(base + (size_t)pos) << 3) | err);
      t++;
      pos += t_len;
      o += (unsigned int)o_len;
    }
    tok_out[t] = o;
    n_tok = t;
  }
  __syncthreads();
  const int nt = n_tok;
  if (nt == 0 || o0 >= n_out) return;
  const unsigned long long room = n_out - o0;
  const unsigned int lim = (unsigned long long)tok_out[nt] < room ? tok_out[nt] : (unsigned int)room;
  for (unsigned int r = (unsigned int)tid; r < lim; r += LZF_SOURCE_WG) {
    int a = 0, b = nt;   // the token with tok_out[a] <= r < tok_out[a + 1]
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (tok_out[mid] <= r) a = mid; else b = mid;
    }
    const int pos = tok_pos[a];
    const unsigned int c = lds[pos];
    const unsigned long long k = o0 + r;
    unsigned int word = LZF_LITERAL;   // a byte of a bad token: stream byte 0, never used (the call fails)
    if (c < 32u) {
      const size_t j = base + (size_t)pos + 1 + (r - tok_out[a]);
      if (j < n) word = LZF_LITERAL | (unsigned int)j;
    } else {
      const int last = pos + ((c >> 5) == 7u ? 2 : 1);
      if (base + (size_t)last < n) {
        const unsigned long long dist = (((c & 31u) << 8) | lds[last]) + 1u;
        if (dist <= k) word = (unsigned int)(k - dist);
      }
    }
    src[k] = word;
  }
}

// (no __restrict__: the words are read and replaced in place)
__global__ __launch_bounds__(256) void lzf_double_kernel(unsigned int* src, unsigned long long n_out, unsigned int* left) {
  const unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_out) return;
  unsigned int s = src[k];
  if (s & LZF_LITERAL) return;
  for (int hop = 0; hop < LZF_HOPS; hop++) {
    s = src[s];   // s < k: an earlier output byte
    if (s & LZF_LITERAL) break;
  }
  src[k] = s;
  if (!(s & LZF_LITERAL)) *left = 1u;
}

__global__ __launch_bounds__(PCDR_WG) void lzf_records_kernel(const unsigned char* __restrict__ in, size_t n,
                                                              const unsigned int* __restrict__ src, unsigned long long n_records,
                                                              PcdBinaryPlan P, unsigned char* __restrict__ records) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PCDR_WG + threadIdx.x;
  if (i >= n_records) return;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int f = 0; f < 4; f++) {
    if (P.src[f] < 0) continue;
    const unsigned long long k = n_records * (unsigned long long)P.src[f] + 4ull * i;   // field-major: the field's block, then the point
    uint32_t x = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const size_t j = src[k + b] & ~LZF_LITERAL;   // resolved: every word is a literal's
      x |= (uint32_t)(j < n ? in[j] : 0u) << (8 * b);
    }
    v[f] = x;
  }
  pcdr_store_record(records + i * (unsigned long long)P.out.step, P.out, pcdr_is_wide(P.out, records), v);
}

// a bracket of two events, the second of which has completed: its time added to *ms
int add_event_ms(hipEvent_t a, hipEvent_t b, double* ms) {
  float t = 0.f;
  LSR_HIP(hipEventElapsedTime(&t, a, b));
  *ms += t;
  return LSR_OK;
}

}  // namespace

int pcd_lzf_inflate(PcdReadState& S, const unsigned char* d_stream, size_t n_stream, size_t n_out, size_t n_records, const PcdBinaryPlan& plan,
                    unsigned char* d_records, unsigned long long file_offset, double* ms, hipStream_t stream) {
  if (n_stream == 0 || n_stream > (size_t)INT32_MAX || n_out == 0 || n_out > (size_t)INT32_MAX || n_records == 0 ||
      n_records * (size_t)plan.rec_bytes != n_out) {
    set_last_error("pcd_lzf_inflate: sizes out of range");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const size_t nb = (n_stream + LZF_BLOCK - 1) / LZF_BLOCK;
  int st;
  if ((st = S.lzf_exit.reserve(nb * LZF_ENTRIES)) || (st = S.lzf_outc.reserve(nb * LZF_ENTRIES)) || (st = S.lzf_entry.reserve(nb)) ||
      (st = S.lzf_out_start.reserve(nb + 1)) || (st = S.lzf_src.reserve(n_out)) || (st = S.lzf_info.reserve(1)) || (st = S.h_lzf_info.reserve(1)))
    return st;
  PcdLzfInfo& H = S.h_lzf_info.p[0];
  std::memset(&H, 0, sizeof(H));
  H.first_error = PCDR_NO_ERROR;
  LSR_HIP(hipMemcpyAsync(S.lzf_info.p, &H, sizeof(H), hipMemcpyHostToDevice, stream));
  if (ms) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I0], stream));
  hipLaunchKernelGGL(lzf_map_kernel, dim3((unsigned)nb), dim3(64), 0, stream, d_stream, n_stream, S.lzf_exit.p, S.lzf_outc.p);
  LSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(lzf_scan_kernel, dim3(1), dim3(LZF_SCAN_WG), 0, stream, S.lzf_exit.p, S.lzf_outc.p, (long long)nb, S.lzf_entry.p,
                     S.lzf_out_start.p, S.lzf_info.p);
  LSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(lzf_source_kernel, dim3((unsigned)nb), dim3(LZF_SOURCE_WG), 0, stream, d_stream, n_stream, (unsigned long long)n_out,
                     S.lzf_entry.p, S.lzf_out_start.p, S.lzf_src.p, S.lzf_info.p);
  LSR_HIP(hipGetLastError());
  if (ms) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I1], stream));
  LSR_HIP(hipMemcpyAsync(&H, S.lzf_info.p, sizeof(H), hipMemcpyDeviceToHost, stream));
  LSR_HIP(hipStreamSynchronize(stream));
  if (ms && (st = add_event_ms(S.ev[PcdReadState::EV_I0], S.ev[PcdReadState::EV_I1], ms))) return st;
  if (H.first_error != PCDR_NO_ERROR) {
    const unsigned int kind = (unsigned int)(H.first_error & 7u);
    const char* why = kind == LZF_ERR_CUT ? "a token that passes the end of the compressed stream"
                                          : (kind == LZF_ERR_TOO_LONG ? "output past uncompressed_size" : "a reference to before the first output byte");
    set_last_error(std::string("PCD body: ") + why + ", token at byte offset " + std::to_string(file_offset + (H.first_error >> 3)));
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (H.total_out != (unsigned long long)n_out) {
    set_last_error("PCD body: the compressed stream inflates to " + std::to_string(H.total_out) + " bytes where uncompressed_size says " +
                   std::to_string(n_out));
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const unsigned nbk = (unsigned)((n_out + 255) / 256);
  for (int pass = 0;; pass++) {
    if (pass == LZF_MAX_PASSES) { set_last_error("PCD body: the references did not resolve"); return LSR_ERR_HIP; }
    if (ms) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I0], stream));
    hipLaunchKernelGGL(lzf_double_kernel, dim3(nbk), dim3(256), 0, stream, S.lzf_src.p, (unsigned long long)n_out, &S.lzf_info.p->unresolved[pass]);
    LSR_HIP(hipGetLastError());
    if (ms) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I1], stream));
    LSR_HIP(hipMemcpyAsync(&H.unresolved[pass], &S.lzf_info.p->unresolved[pass], sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
    LSR_HIP(hipStreamSynchronize(stream));
    if (ms && (st = add_event_ms(S.ev[PcdReadState::EV_I0], S.ev[PcdReadState::EV_I1], ms))) return st;
    if (!H.unresolved[pass]) break;
  }
  if (ms) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I0], stream));
  hipLaunchKernelGGL(lzf_records_kernel, dim3((unsigned)((n_records + PCDR_WG - 1) / PCDR_WG)), dim3(PCDR_WG), 0, stream, d_stream, n_stream,
                     S.lzf_src.p, (unsigned long long)n_records, plan, d_records);
  LSR_HIP(hipGetLastError());
  if (ms) {
    LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_I1], stream));
    LSR_HIP(hipStreamSynchronize(stream));
    if ((st = add_event_ms(S.ev[PcdReadState::EV_I0], S.ev[PcdReadState::EV_I1], ms))) return st;
  }
  return LSR_OK;
}

}  // namespace lsr
