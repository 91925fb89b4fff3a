// Records in HBM -> the body of an ASCII .pcd file, the bytes pcl::io::savePCDFileASCII writes (the per-float text is
// csrc/pcd_format.hpp, integer arithmetic only).  Three launches, every byte with one writer, the result fixed whatever the scheduling:
// no atomics, no workgroup waits for another.
//   pcd_length_kernel   one record per thread: the length of its line; per-workgroup sums
//   pcd_scan_kernel     ONE workgroup: exclusive scan of the workgroup sums in 64 bits, the total behind it
//   pcd_write_kernel    one record per thread again: digits once more (cheap next to scattered byte stores to HBM), an in-workgroup scan
//                       of the line lengths, the lines written into an LDS image of the workgroup's text (256 x 60 B at most), and the
//                       image streamed to its place with aligned dword stores — the image is laid out in LDS at the global address's
//                       own offset inside a dword, so aligned words of the one are aligned words of the other; the ragged first and
//                       last word go out byte by byte (their other bytes belong to the neighbouring workgroups)
#include "pcd_format.hpp"
#include "pcd_text.hpp"

namespace lsr {

namespace {

__device__ inline unsigned int pcd_load_bits(const unsigned char* rec, int off) {
  return *reinterpret_cast<const unsigned int*>(rec + off);   // records and offsets are 4-byte aligned (checked by the entry points)
}

__global__ __launch_bounds__(PCD_WG) void pcd_length_kernel(const unsigned char* __restrict__ records, int n, PcdFields L,
                                                            unsigned int* __restrict__ block_sums) {
  __shared__ unsigned int wave_sum[PCD_WG / 64];
  const long long i = (long long)blockIdx.x * PCD_WG + threadIdx.x;
  unsigned int len = 0;
  if (i < n) {
    const unsigned char* rec = records + (size_t)i * (size_t)L.step;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < L.n_fields) len += (unsigned int)pcd_float_length(pcd_load_bits(rec, L.off[k])) + 1u;   // + the blank or the newline
  }
  for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int w = 0; w < PCD_WG / 64; w++) s += wave_sum[w];
    block_sums[blockIdx.x] = s;
  }
}

constexpr int PCD_SCAN_WG = 1024;

__global__ __launch_bounds__(PCD_SCAN_WG) void pcd_scan_kernel(const unsigned int* __restrict__ sums, int nb,
                                                               unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long wave_tot[PCD_SCAN_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long chunk = ((long long)nb + PCD_SCAN_WG - 1) / PCD_SCAN_WG;
  const long long lo = min((long long)tid * chunk, (long long)nb), hi = min(lo + chunk, (long long)nb);
  unsigned long long s = 0;
  for (long long j = lo; j < hi; j++) s += sums[j];
  unsigned long long inc = s;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  unsigned long long before = 0;
  for (int w = 0; w < wave; w++) before += wave_tot[w];
  unsigned long long run = before + inc - s;
  for (long long j = lo; j < hi; j++) {
    offsets[j] = run;
    run += sums[j];
  }
  if (tid == PCD_SCAN_WG - 1) offsets[nb] = run;   // the last thread's chunk ends at nb (or is empty behind it): run is the total
}

constexpr int PCD_IMAGE_WORDS = (PCD_WG * PCD_MAX_LINE_BYTES + 3) / 4 + 1;   // the image plus up to three bytes of lead

__global__ __launch_bounds__(PCD_WG) void pcd_write_kernel(const unsigned char* __restrict__ records, int n, PcdFields L,
                                                           const unsigned long long* __restrict__ offsets, unsigned char* __restrict__ text) {
  __shared__ unsigned int image[PCD_IMAGE_WORDS];
  __shared__ int wave_tot[PCD_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = (long long)blockIdx.x * PCD_WG + tid;
  PcdField F[4];
  int len = 0;
  if (i < n) {
    const unsigned char* rec = records + (size_t)i * (size_t)L.step;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < L.n_fields) {
        F[k] = pcd_decompose(pcd_load_bits(rec, L.off[k]));
        len += pcd_field_length(F[k]) + 1;
      }
  }
  int inc = len;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < PCD_WG / 64; w++) {
    if (w < wave) before += wave_tot[w];
    total += wave_tot[w];
  }
  unsigned char* dst = text + offsets[blockIdx.x];
  const int shift = (int)((uintptr_t)dst & 3);
  if (i < n) {
    char* p = reinterpret_cast<char*>(image) + shift + before + inc - len;   // ends at most at byte 3 + 256 * 60 of the image
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < L.n_fields) {
        p += pcd_field_emit(F[k], p);
        *p++ = (k + 1 < L.n_fields) ? ' ' : '\n';
      }
  }
  __syncthreads();
  // image bytes [shift, span) go to dst - shift + [shift, span): word w of the image is the aligned word w behind dst - shift
  // (never past the room the length pass measured for this workgroup, should the records have changed in between)
  const unsigned long long room = offsets[blockIdx.x + 1] - offsets[blockIdx.x];
  if ((unsigned long long)total > room) total = (int)room;
  const int span = shift + total, n_words = (span + 3) >> 2;
  unsigned char* g0 = dst - shift;
  const unsigned char* img = reinterpret_cast<const unsigned char*>(image);
  for (int w = tid; w < n_words; w += PCD_WG) {
    const int lo = 4 * w, hi = lo + 4;
    if (lo >= shift && hi <= span) {
      reinterpret_cast<unsigned int*>(g0)[w] = image[w];
    } else {
      const int a = lo > shift ? lo : shift, b = hi < span ? hi : span;
      for (int c = a; c < b; c++) g0[c] = img[c];
    }
  }
}

}  // namespace

int pcd_header_text(size_t n, bool with_intensity, char* out, const char* data_word) {
  const int len = std::snprintf(out, PCD_MAX_HEADER_BYTES,
                                "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z%s\nSIZE 4 4 4%s\nTYPE F F F%s\nCOUNT 1 1 1%s\n"
                                "WIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA %s\n",
                                with_intensity ? " intensity" : "", with_intensity ? " 4" : "", with_intensity ? " F" : "",
                                with_intensity ? " 1" : "", n, n, data_word);
  return len;
}

int pcd_text_lengths(const void* d_records, size_t n, const PcdFields& F, unsigned int* d_block_sums, unsigned long long* d_offsets,
                     hipStream_t stream) {
  if (n == 0 || n > (size_t)INT32_MAX) { set_last_error("pcd_text_lengths: record count out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const int nb = (int)pcd_blocks(n);
  hipLaunchKernelGGL(pcd_length_kernel, dim3(nb), dim3(PCD_WG), 0, stream, static_cast<const unsigned char*>(d_records), (int)n, F, d_block_sums);
  LSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(pcd_scan_kernel, dim3(1), dim3(PCD_SCAN_WG), 0, stream, d_block_sums, nb, d_offsets);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_text_write(const void* d_records, size_t n, const PcdFields& F, const unsigned long long* d_offsets, unsigned char* d_text,
                   hipStream_t stream) {
  if (n == 0 || n > (size_t)INT32_MAX) { set_last_error("pcd_text_write: record count out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  const int nb = (int)pcd_blocks(n);
  hipLaunchKernelGGL(pcd_write_kernel, dim3(nb), dim3(PCD_WG), 0, stream, static_cast<const unsigned char*>(d_records), (int)n, F, d_offsets,
                     d_text);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

}  // namespace lsr
