// A .pcd body in HBM -> records of an lsr_pc2_layout (the inverse of csrc/pcd_text.hip; the per-token arithmetic and the line machine are
// csrc/pcd_parse.hpp, integer arithmetic only).  ASCII: four launches, every slot and every record with one writer, the result fixed
// whatever the scheduling; the only atomics are the error word (a minimum: the earliest bad line wins) and the unresolved count.
//   pcdr_line_kernel    each thread walks PCDR_RUN bytes (16-byte loads, single bytes at a ragged head and tail) and forms what the run does
//                       to the two-state line machine; the workgroup composes its threads' runs in the wave and through LDS
//   pcdr_scan_kernel    ONE workgroup: the workgroups' runs composed in order, the text entered in state 0 -> per workgroup its entry
//                       state and the number of point lines in front of it (64 bits), the total behind them
//   pcdr_index_kernel   the same walk with the known entry state: the offset of every point line's first byte into its slot
//   pcdr_parse_kernel   one point line per thread: tokens cut at blanks, those of x y z [intensity] turned into bits, the record stored
//                       whole (bytes outside the fields zero); a line's tokens differ in length, so lanes diverge inside a token — the
//                       alternative, a lane per token, would leave a quarter of the lanes to lines of x y z only and buys nothing for
//                       the stores; records of {32; 0,4,8,16} on a 16-byte boundary go out as two 16-byte stores per lane, any other
//                       layout as one dword per field and padding word (DESIGN.md 4 "Reading PCD on the device")
// Binary: pcdr_binary_kernel, a record per thread, dword loads when body, record size and offsets allow, single bytes otherwise.
#include <cerrno>
#include <cstdlib>

#include "pcd_read.hpp"

namespace lsr {

namespace {

__device__ inline PcdRun pcdr_shfl_up(const PcdRun& r, int d) {
  PcdRun o;
  o.f = __shfl_up(r.f, d, 64);
  o.c0 = __shfl_up(r.c0, d, 64);
  o.c1 = __shfl_up(r.c1, d, 64);
  return o;
}

// inclusive scan of the wave's runs in lane order
__device__ inline PcdRun pcdr_wave_scan(PcdRun r, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const PcdRun up = pcdr_shfl_up(r, d);
    if (lane >= d) r = pcd_run_compose(up, r);
  }
  return r;
}

__global__ __launch_bounds__(PCDR_WG) void pcdr_line_kernel(const unsigned char* __restrict__ text, size_t n, PcdRun* __restrict__ wg_runs) {
  __shared__ PcdRun wave_tot[PCDR_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  size_t a, b;
  pcd_run_bounds(text, n, PCDR_RUN, (size_t)blockIdx.x * PCDR_WG + tid, &a, &b);
  const PcdRun inc = pcdr_wave_scan(pcd_run_of(text, a, b), lane);
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  if (tid == 0) {
    PcdRun r = wave_tot[0];
    for (int w = 1; w < PCDR_WG / 64; w++) r = pcd_run_compose(r, wave_tot[w]);
    wg_runs[blockIdx.x] = r;
  }
}

constexpr int PCDR_SCAN_WG = 1024;

__global__ __launch_bounds__(PCDR_SCAN_WG) void pcdr_scan_kernel(const PcdRun* __restrict__ wg_runs, long long nb,
                                                                 unsigned long long* __restrict__ first_slot,
                                                                 unsigned char* __restrict__ entry_state) {
  __shared__ PcdRun wave_tot[PCDR_SCAN_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long chunk = (nb + PCDR_SCAN_WG - 1) / PCDR_SCAN_WG;
  const long long lo = min((long long)tid * chunk, nb), hi = min(lo + chunk, nb);
  PcdRun mine = pcd_run_identity();
  for (long long j = lo; j < hi; j++) mine = pcd_run_compose(mine, wg_runs[j]);
  const PcdRun inc = pcdr_wave_scan(mine, lane);
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  PcdRun before = pcd_run_identity();
  for (int w = 0; w < wave; w++) before = pcd_run_compose(before, wave_tot[w]);
  PcdRun prev = pcdr_shfl_up(inc, 1);
  if (lane == 0) prev = pcd_run_identity();
  before = pcd_run_compose(before, prev);
  // the text is entered in state 0
  unsigned int state = before.f & 1u;
  unsigned long long slot = before.c0;
  for (long long j = lo; j < hi; j++) {
    const PcdRun r = wg_runs[j];
    first_slot[j] = slot;
    entry_state[j] = (unsigned char)state;
    slot += state ? r.c1 : r.c0;
    state = (r.f >> state) & 1u;
  }
  if (tid == PCDR_SCAN_WG - 1) first_slot[nb] = slot;   // the last thread's chunk ends at nb (or is empty behind it)
}

__global__ __launch_bounds__(PCDR_WG) void pcdr_index_kernel(const unsigned char* __restrict__ text, size_t n,
                                                             const unsigned long long* __restrict__ first_slot,
                                                             const unsigned char* __restrict__ entry_state, unsigned long long n_keep,
                                                             unsigned int* __restrict__ line_start) {
  __shared__ PcdRun wave_tot[PCDR_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  size_t a, b;
  pcd_run_bounds(text, n, PCDR_RUN, (size_t)blockIdx.x * PCDR_WG + tid, &a, &b);
  const PcdRun inc = pcdr_wave_scan(pcd_run_of(text, a, b), lane);
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  PcdRun before = pcd_run_identity();
  for (int w = 0; w < wave; w++) before = pcd_run_compose(before, wave_tot[w]);
  PcdRun prev = pcdr_shfl_up(inc, 1);
  if (lane == 0) prev = pcd_run_identity();
  before = pcd_run_compose(before, prev);
  const unsigned int s_in = entry_state[blockIdx.x];
  unsigned long long slot = first_slot[blockIdx.x] + (s_in ? before.c1 : before.c0);
  if (slot >= n_keep) return;   // lines behind POINTS are not looked at
  const unsigned int state = (before.f >> s_in) & 1u;
  pcd_run_index(text, a, b, state, [&](size_t i) {
    if (slot < n_keep) line_start[slot] = (unsigned int)i;
    slot++;
  });
}

__global__ __launch_bounds__(PCDR_WG) void pcdr_parse_kernel(const unsigned char* __restrict__ text, size_t n,
                                                             const unsigned int* __restrict__ line_start, unsigned long long n_lines,
                                                             PcdAsciiPlan P, unsigned char* __restrict__ records,
                                                             unsigned char* __restrict__ flags, PcdReadStatus* __restrict__ status) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PCDR_WG + threadIdx.x;
  if (i >= n_lines) return;
  const size_t p = line_start[i];
  const size_t lim = min(n, p + (size_t)PCDR_MAX_LINE + 1);   // one byte more than a line may have
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  unsigned int unresolved = 0, err = 0;
  int t = 0;
  size_t j = p;
  for (;;) {
    while (j < lim && pcd_is_blank(text[j])) j++;
    if (j >= lim || text[j] == '\n') break;
    const size_t s = j;
    while (j < lim && !pcd_is_blank(text[j]) && text[j] != '\n') j++;
    int k = -1;
#pragma unroll
    for (int m = 0; m < 4; m++)
      if (P.tok[m] == t) k = m;
    if (k >= 0) {
      uint32_t bits = 0;
      const int st = pcd_parse_float(text + s, (int)(j - s), &bits);
      if (st == PCD_TOK_BAD) err = PCDR_ERR_TOKEN;
      if (st == PCD_TOK_UNRESOLVED) unresolved |= 1u << k;
#pragma unroll
      for (int m = 0; m < 4; m++)
        if (m == k) v[m] = bits;
    }
    t++;
  }
  if (t < P.n_tokens) err = PCDR_ERR_SHORT;
  if (j == p + (size_t)PCDR_MAX_LINE + 1) err = PCDR_ERR_TOO_LONG;   // no newline within PCDR_MAX_LINE bytes of the line's first
  if (err) {
    atomicMin(&status->first_error, ((unsigned long long)p << 3) | err);
    return;
  }
  pcdr_store_record(records + i * (unsigned long long)P.out.step, P.out, pcdr_is_wide(P.out, records), v);
  flags[i] = (unsigned char)unresolved;
  if (unresolved) atomicAdd(&status->unresolved, (unsigned int)__popc(unresolved));
}

__global__ __launch_bounds__(PCDR_WG) void pcdr_binary_kernel(const unsigned char* __restrict__ body, unsigned long long n_records,
                                                              PcdBinaryPlan P, unsigned char* __restrict__ records) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PCDR_WG + threadIdx.x;
  if (i >= n_records) return;
  const unsigned char* src = body + i * (unsigned long long)P.rec_bytes;
  // the same in every lane: the body starts wherever the header ends
  const bool aligned = (((uintptr_t)body | P.rec_bytes | (unsigned)P.src[0] | (unsigned)P.src[1] | (unsigned)P.src[2] |
                         (unsigned)(P.src[3] < 0 ? 0 : P.src[3])) & 3u) == 0;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (P.src[k] < 0) continue;
    const unsigned char* f = src + P.src[k];
    if (aligned) v[k] = *reinterpret_cast<const uint32_t*>(f);
    else v[k] = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
  }
  pcdr_store_record(records + i * (unsigned long long)P.out.step, P.out, pcdr_is_wide(P.out, records), v);
}

// ---- the header, on the host -----------------------------------------------------------------------------------------------------------
int header_bad(const std::string& why) {
  set_last_error("PCD header: " + why);
  return LSR_ERR_INVALID_ARGUMENT;
}

bool header_u64(const std::string& w, uint64_t* v) {
  if (w.empty() || w.size() > 19) return false;
  uint64_t x = 0;
  for (char c : w) {
    if (c < '0' || c > '9') return false;
    x = x * 10 + (uint64_t)(c - '0');
  }
  *v = x;
  return true;
}

}  // namespace

int pcd_parse_header(const void* bytes, size_t n_bytes, PcdHeader* H, bool* incomplete, bool take_compressed) {
  if (incomplete) *incomplete = false;
  const char* text = static_cast<const char*>(bytes);
  std::vector<std::string> names, types;
  std::vector<uint64_t> sizes, counts;
  bool have_version = false, have_fields = false, have_size = false, have_type = false, have_count = false, have_width = false,
       have_height = false, have_points = false, have_data = false;
  uint64_t width = 0, height = 1, points = 0;
  double viewpoint[7] = {0, 0, 0, 1, 0, 0, 0};
  int data_kind = -1;
  size_t pos = 0, data_offset = 0;
  std::vector<std::string> words;
  while (!have_data) {
    const void* nl = pos < n_bytes ? std::memchr(text + pos, '\n', n_bytes - pos) : nullptr;
    if (!nl) {
      if (incomplete) *incomplete = true;
      return header_bad("header incomplete (no DATA line within the bytes given)");
    }
    const size_t end = (size_t)(static_cast<const char*>(nl) - text);
    words.clear();
    for (size_t i = pos; i < end;) {
      while (i < end && pcd_is_blank((unsigned char)text[i])) i++;
      size_t s = i;
      while (i < end && !pcd_is_blank((unsigned char)text[i])) i++;
      if (i > s) words.emplace_back(text + s, i - s);
    }
    pos = end + 1;
    if (words.empty() || words[0][0] == '#') continue;
    const std::string& key = words[0];
    const size_t nv = words.size() - 1;
    auto numbers = [&](std::vector<uint64_t>* out) {
      out->clear();
      for (size_t i = 1; i < words.size(); i++) {
        uint64_t v;
        if (!header_u64(words[i], &v)) return false;
        out->push_back(v);
      }
      return !out->empty();
    };
    auto one = [&](uint64_t* v) { return nv == 1 && header_u64(words[1], v); };
    if (key == "VERSION") {
      if (nv != 1) return header_bad("malformed VERSION");
      have_version = true;
    } else if (key == "FIELDS" || key == "COLUMNS") {
      if (nv == 0) return header_bad("malformed FIELDS");
      names.assign(words.begin() + 1, words.end());
      have_fields = true;
    } else if (key == "SIZE") {
      if (!numbers(&sizes)) return header_bad("malformed SIZE");
      have_size = true;
    } else if (key == "TYPE") {
      if (nv == 0) return header_bad("malformed TYPE");
      types.assign(words.begin() + 1, words.end());
      have_type = true;
    } else if (key == "COUNT") {
      if (!numbers(&counts)) return header_bad("malformed COUNT");
      have_count = true;
    } else if (key == "WIDTH") {
      if (!one(&width)) return header_bad("malformed WIDTH");
      have_width = true;
    } else if (key == "HEIGHT") {
      if (!one(&height)) return header_bad("malformed HEIGHT");
      have_height = true;
    } else if (key == "POINTS") {
      if (!one(&points)) return header_bad("malformed POINTS");
      have_points = true;
    } else if (key == "VIEWPOINT") {
      if (nv != 7) return header_bad("malformed VIEWPOINT");
      for (int i = 0; i < 7; i++) {
        char* e = nullptr;
        viewpoint[i] = std::strtod(words[1 + i].c_str(), &e);
        if (e == words[1 + i].c_str() || *e) return header_bad("malformed VIEWPOINT");
      }
    } else if (key == "DATA") {
      if (nv != 1) return header_bad("malformed DATA");
      data_kind = words[1] == "ascii" ? 0 : (words[1] == "binary" ? 1 : (words[1] == "binary_compressed" ? 2 : -1));
      if (data_kind < 0) return header_bad("unknown DATA kind '" + words[1] + "'");
      have_data = true;
      data_offset = pos;
    }
    // any other entry is passed over
  }
  (void)have_height;
  if (!have_version) return header_bad("no VERSION entry");
  if (!have_fields) return header_bad("no FIELDS entry");
  if (!have_size) return header_bad("no SIZE entry");
  if (!have_type) return header_bad("no TYPE entry");
  if (!have_width) return header_bad("no WIDTH entry");
  const size_t nf = names.size();
  if (!have_count) counts.assign(nf, 1);
  if (sizes.size() != nf || types.size() != nf || counts.size() != nf) return header_bad("FIELDS, SIZE, TYPE and COUNT differ in length");
  if (nf > 4096) return header_bad("more than 4096 fields");
  uint64_t tok = 0, off = 0;
  int f_tok[4] = {-1, -1, -1, -1}, f_off[4] = {-1, -1, -1, -1};
  bool f_float[4] = {true, true, true, true};
  static const char* wanted[4] = {"x", "y", "z", "intensity"};
  for (size_t i = 0; i < nf; i++) {
    const uint64_t s = sizes[i], c = counts[i];
    if (!(s == 1 || s == 2 || s == 4 || s == 8)) return header_bad("a SIZE that is not 1, 2, 4 or 8");
    if (!(types[i] == "I" || types[i] == "U" || types[i] == "F")) return header_bad("a TYPE that is not I, U or F");
    if (c < 1 || c > (1u << 20)) return header_bad("a COUNT outside 1 .. 1 << 20");
    for (int k = 0; k < 4; k++)
      if (names[i] == wanted[k]) {
        if (f_tok[k] >= 0) return header_bad(std::string("field ") + wanted[k] + " appears twice");
        if (c != 1) return header_bad(std::string("field ") + wanted[k] + " with a COUNT other than 1");
        f_tok[k] = (int)tok;
        f_off[k] = (int)off;
        f_float[k] = s == 4 && types[i] == "F";
      }
    tok += c;
    off += s * c;
    if (tok > (1u << 24) || off > (1u << 27)) return header_bad("a record of more than 1 << 24 values or 1 << 27 bytes");
  }
  if (f_tok[0] < 0 || f_tok[1] < 0 || f_tok[2] < 0) return header_bad("x, y and z are required");
  uint64_t wh = 0;
  if (__builtin_mul_overflow(width, height, &wh)) return header_bad("WIDTH * HEIGHT overflows");
  if (!have_points) points = wh;
  if (points != wh) return header_bad("POINTS disagrees with WIDTH * HEIGHT");
  if (points == 0) return header_bad("POINTS is 0");
  if (points > (uint64_t)INT32_MAX) { set_last_error("PCD header: more than INT32_MAX points"); return LSR_ERR_INDEX_OVERFLOW; }
  lsr_pcd_info& I = H->info;
  I.n_points = points; I.width = width; I.height = height; I.data_offset = data_offset;
  I.point_step = (uint32_t)off; I.data_kind = data_kind; I.has_intensity = f_tok[3] >= 0 ? 1 : 0; I.n_fields = (int32_t)nf;
  std::memcpy(I.viewpoint, viewpoint, sizeof(viewpoint));
  for (int k = 0; k < 4; k++) { H->tok[k] = f_tok[k]; H->src[k] = f_off[k]; }
  H->n_tokens = (int)tok;
  for (int k = 0; k < 4; k++)
    if (!f_float[k]) {
      set_last_error(std::string("PCD header: field ") + wanted[k] + " is not a 4-byte float (SIZE 4, TYPE F)");
      return LSR_ERR_NOT_IMPLEMENTED;
    }
  if (data_kind == 2 && !take_compressed) { set_last_error("PCD header: DATA binary_compressed is not read"); return LSR_ERR_NOT_IMPLEMENTED; }
  return LSR_OK;
}

int pcd_read_lines(const unsigned char* d_text, size_t n, PcdRun* d_wg_runs, unsigned long long* d_first_slot, unsigned char* d_entry_state,
                   hipStream_t stream) {
  if (n == 0 || n >= ((size_t)1 << 32)) { set_last_error("pcd_read_lines: text size out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t nb = pcdr_blocks(d_text, n);
  hipLaunchKernelGGL(pcdr_line_kernel, dim3((unsigned)nb), dim3(PCDR_WG), 0, stream, d_text, n, d_wg_runs);
  LSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(pcdr_scan_kernel, dim3(1), dim3(PCDR_SCAN_WG), 0, stream, d_wg_runs, (long long)nb, d_first_slot, d_entry_state);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_read_index(const unsigned char* d_text, size_t n, const unsigned long long* d_first_slot, const unsigned char* d_entry_state,
                   size_t n_keep, unsigned int* d_line_start, hipStream_t stream) {
  if (n == 0 || n >= ((size_t)1 << 32)) { set_last_error("pcd_read_index: text size out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t nb = pcdr_blocks(d_text, n);
  hipLaunchKernelGGL(pcdr_index_kernel, dim3((unsigned)nb), dim3(PCDR_WG), 0, stream, d_text, n, d_first_slot, d_entry_state,
                     (unsigned long long)n_keep, d_line_start);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_read_parse(const unsigned char* d_text, size_t n, const unsigned int* d_line_start, size_t n_lines, const PcdAsciiPlan& plan,
                   unsigned char* d_records, unsigned char* d_flags, PcdReadStatus* d_status, hipStream_t stream) {
  if (n_lines == 0 || n_lines > (size_t)INT32_MAX) { set_last_error("pcd_read_parse: line count out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t nb = (n_lines + PCDR_WG - 1) / PCDR_WG;
  hipLaunchKernelGGL(pcdr_parse_kernel, dim3((unsigned)nb), dim3(PCDR_WG), 0, stream, d_text, n, d_line_start, (unsigned long long)n_lines, plan,
                     d_records, d_flags, d_status);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_read_binary(const unsigned char* d_body, size_t n_records, const PcdBinaryPlan& plan, unsigned char* d_records, hipStream_t stream) {
  if (n_records == 0 || n_records > (size_t)INT32_MAX) { set_last_error("pcd_read_binary: record count out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t nb = (n_records + PCDR_WG - 1) / PCDR_WG;
  hipLaunchKernelGGL(pcdr_binary_kernel, dim3((unsigned)nb), dim3(PCDR_WG), 0, stream, d_body, (unsigned long long)n_records, plan, d_records);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

}  // namespace lsr
