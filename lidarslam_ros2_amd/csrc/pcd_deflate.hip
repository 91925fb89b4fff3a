// DATA binary and DATA binary_compressed bodies from records in HBM: two gather kernels and a parallel LZF compressor (the token format
// is liblzf's, restated in include/lidarslam_reg.h).  The stream is a PURE FUNCTION OF THE IMAGE — not of the piece size, of where the
// buffers live, of the object or of the call.  THE RULE (restated on the host in tests/pcd_write_numpy.py):
//   The image is cut into chunks of DFL_CHUNK = 4096 bytes (the last may be shorter).  A chunk is compressed on its own: no reference
//   reaches before the chunk's first byte, so the chunks' streams, back to back, are one valid LZF stream.
//   candidate(i), for a position i with at least three bytes left in the chunk: the NEAREST earlier position p < i of the chunk whose
//   three bytes equal the three at i (compared exactly, no hash).  length(i): how far the bytes behind p and behind i go on being equal
//   (p + length may pass i: a repeating pattern), at most 264 and at most up to the chunk's end.
//   The parse is greedy from the chunk's first byte: with a candidate, a reference (length, distance i - p) and on by `length`; without,
//   the byte is a literal and on by one.  Literals go out in runs of at most 32; a run ends at a reference and at the chunk's end.
//   A reference of length <= 8 takes the two-byte form, from 9 on the three-byte form.
// A chunk's stream has at most c + ceil(c / 32) bytes for a chunk of c bytes (a reference is shorter than what it stands for by at
// least the control byte the literal run behind it may add).
//   pcd_pack_kernel / pcd_image_kernel   one record per thread: its three or four fields as a packed record / into the field-major image
//   dfl_chunk_kernel    a workgroup per chunk, everything in LDS (52 KiB: three workgroups on a CU's 160 KiB):
//                       1. (3-byte key << 12 | position) of every position, bitonic sort — the predecessor in sorted order with the
//                          same key is the nearest earlier occurrence;  2. every position's length, compared in LDS four bytes a step;
//                       3. next[i] = i + (length or 1): the positions the greedy parse visits are those reachable from 0, marked by
//                          pointer doubling (12 rounds);  4. a max-scan gives every visited literal the start of its run (hence where
//                          the control bytes fall), a sum-scan every token's offset;  5. every visited position writes its own token
//                          into an LDS image of the chunk's stream, stored to the chunk's slot with dword stores
//   dfl_scan_kernel     ONE workgroup: exclusive scan of the chunks' stream lengths in 64 bits, the total behind it
//   dfl_compact_kernel  a workgroup per chunk: its slot to its place in the stream, as pcd_write_kernel stores its text (the image laid
//                       out in LDS at the destination's offset inside a dword, aligned dword stores, ragged ends byte by byte)
// Every byte has one writer and no workgroup waits for another: the result is fixed whatever the scheduling.  No atomics.
#include "pcd_deflate.hpp"

namespace lsr {

namespace {

constexpr int DFL_WG = 256;
constexpr int DFL_PER = DFL_CHUNK / DFL_WG;   // positions per thread
constexpr int DFL_POS_BITS = 12;
constexpr unsigned int DFL_NO_KEY = 1u << 24;   // above every 3-byte key: a position with fewer than three bytes behind it
constexpr unsigned short DFL_NONE = 0xFFFF;
static_assert((1 << DFL_POS_BITS) == DFL_CHUNK && DFL_CHUNK % (4 * DFL_WG) == 0 && DFL_SLOT % 4 == 0, "chunk geometry");
// what lies in the sort's memory (8 * DFL_CHUNK bytes) once the candidates are out
constexpr int DFL_AT_JUMP = 0;                                  // unsigned short [DFL_CHUNK + 1]
constexpr int DFL_AT_REACH = 2 * DFL_CHUNK + 256;               // unsigned char [DFL_CHUNK + 1]
constexpr int DFL_AT_OUT = DFL_AT_REACH + DFL_CHUNK + 256;      // unsigned char [DFL_SLOT + 4]
static_assert(DFL_AT_OUT + DFL_SLOT + 4 <= 8 * DFL_CHUNK && DFL_AT_OUT % 4 == 0, "the views fit in the sort's memory");

__device__ inline unsigned int dfl_load_bits(const unsigned char* rec, int off) {
  return *reinterpret_cast<const unsigned int*>(rec + off);   // records and offsets are 4-byte aligned (checked by the entry points)
}

// the four bytes from byte q of the word array on (little endian; word (q >> 2) + 1 exists)
__device__ inline unsigned int dfl_load4(const unsigned int* w, int q) {
  const unsigned long long both = ((unsigned long long)w[(q >> 2) + 1] << 32) | (unsigned long long)w[q >> 2];
  return (unsigned int)(both >> (8 * (q & 3)));
}

__global__ __launch_bounds__(256) void pcd_pack_kernel(const unsigned char* __restrict__ records, int n, PcdFields L,
                                                       unsigned int* __restrict__ packed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned char* rec = records + (size_t)i * (size_t)L.step;
  unsigned int* dst = packed + (size_t)i * (size_t)L.n_fields;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k < L.n_fields) dst[k] = dfl_load_bits(rec, L.off[k]);
}

__global__ __launch_bounds__(256) void pcd_image_kernel(const unsigned char* __restrict__ records, int n, PcdFields L,
                                                        unsigned int* __restrict__ image) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned char* rec = records + (size_t)i * (size_t)L.step;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k < L.n_fields) image[(size_t)k * (size_t)n + (size_t)i] = dfl_load_bits(rec, L.off[k]);
}

__global__ __launch_bounds__(DFL_WG) void dfl_chunk_kernel(const unsigned char* __restrict__ image, size_t n_image,
                                                           unsigned char* __restrict__ slots, unsigned int* __restrict__ chunk_bytes) {
  __shared__ unsigned int data_w[DFL_CHUNK / 4 + 2];   // the chunk, zeros behind it
  __shared__ unsigned long long keys[DFL_CHUNK];
  __shared__ unsigned short cand[DFL_CHUNK], mlen[DFL_CHUNK];
  __shared__ int wave_max[DFL_WG / 64];
  __shared__ unsigned int wave_sum[DFL_WG / 64];
  __shared__ unsigned int total_s;
  const unsigned char* data = reinterpret_cast<const unsigned char*>(data_w);
  unsigned short* jump = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(keys) + DFL_AT_JUMP);
  unsigned char* reach = reinterpret_cast<unsigned char*>(keys) + DFL_AT_REACH;
  unsigned char* out = reinterpret_cast<unsigned char*>(keys) + DFL_AT_OUT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)blockIdx.x * DFL_CHUNK;
  const int L = (int)(n_image - base < (size_t)DFL_CHUNK ? n_image - base : (size_t)DFL_CHUNK);

  // the chunk into LDS (the image and a chunk's first byte are 4-byte aligned)
  const unsigned int* src = reinterpret_cast<const unsigned int*>(image + base);
  for (int w = tid; w < DFL_CHUNK / 4 + 2; w += DFL_WG) {
    const int lo = 4 * w;
    unsigned int v = 0;
    if (lo + 4 <= L) {
      v = src[w];
    } else {
      for (int b = 0; b < 4; b++)
        if (lo + b < L) v |= (unsigned int)image[base + (size_t)(lo + b)] << (8 * b);
    }
    data_w[w] = v;
  }
  __syncthreads();

  // 1. candidates: sort (key, position); positions are distinct, so are the entries
  for (int i = tid; i < DFL_CHUNK; i += DFL_WG) {
    const unsigned int key = i + 3 <= L ? ((unsigned int)data[i] << 16) | ((unsigned int)data[i + 1] << 8) | (unsigned int)data[i + 2] : DFL_NO_KEY;
    keys[i] = ((unsigned long long)key << DFL_POS_BITS) | (unsigned long long)i;
  }
#pragma nounroll
  for (int k = 2; k <= DFL_CHUNK; k <<= 1)
#pragma nounroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < DFL_CHUNK / 2; t += DFL_WG) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) {
          keys[i] = b;
          keys[l] = a;
        }
      }
    }
  __syncthreads();
  for (int r = tid; r < DFL_CHUNK; r += DFL_WG) {
    const unsigned long long e = keys[r];
    const unsigned int key = (unsigned int)(e >> DFL_POS_BITS);
    unsigned short c = DFL_NONE;
    if (r > 0 && key < DFL_NO_KEY) {
      const unsigned long long p = keys[r - 1];
      if ((unsigned int)(p >> DFL_POS_BITS) == key) c = (unsigned short)(p & (DFL_CHUNK - 1));
    }
    cand[e & (DFL_CHUNK - 1)] = c;
  }
  __syncthreads();   // the sort's memory is free from here on

  // 2. lengths, next
  for (int i = tid; i < DFL_CHUNK; i += DFL_WG) {
    int len = 0;
    const int p = cand[i];
    if (i < L && p != DFL_NONE) {
      const int lim = L - i < DFL_MAX_LEN ? L - i : DFL_MAX_LEN;
      len = 3;
      while (len < lim) {   // four bytes a step; what lies behind the chunk reads as zeros and is cut off by lim
        const unsigned int x = dfl_load4(data_w, p + len) ^ dfl_load4(data_w, i + len);
        if (x) {
          len += __builtin_ctz(x) >> 3;
          break;
        }
        len += 4;
      }
      if (len > lim) len = lim;
    }
    mlen[i] = (unsigned short)len;
    jump[i] = (unsigned short)(i < L ? i + (len ? len : 1) : DFL_CHUNK);
    reach[i] = i == 0 ? 1 : 0;
  }
  if (tid == 0) {
    jump[DFL_CHUNK] = DFL_CHUNK;
    reach[DFL_CHUNK] = 0;
  }

  // 3. the positions the parse visits: after round r every position less than 2^(r + 1) steps from 0 is marked
#pragma nounroll
  for (int round = 0; round < DFL_POS_BITS; round++) {
    __syncthreads();
    unsigned short to[DFL_PER], to2[DFL_PER];
    unsigned char on[DFL_PER];
#pragma unroll
    for (int j = 0; j < DFL_PER; j++) {
      const int i = tid + j * DFL_WG;
      to[j] = jump[i];
      on[j] = reach[i];
      to2[j] = jump[to[j]];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DFL_PER; j++) {
      const int i = tid + j * DFL_WG;
      if (on[j]) reach[to[j]] = 1;   // several writers, one value
      jump[i] = to2[j];
    }
  }
  __syncthreads();

  // 4. token sizes: thread t owns positions 16 t .. 16 t + 15.  kind: 0 not visited, 1 literal, 2 reference
  const int i0 = tid * DFL_PER;
  unsigned char kind[DFL_PER];
  unsigned short len16[DFL_PER];
#pragma unroll
  for (int j = 0; j < DFL_PER; j++) {
    const int i = i0 + j;
    len16[j] = mlen[i];
    kind[j] = (i < L && reach[i]) ? (len16[j] ? 2 : 1) : 0;
  }
  const bool lit_before = i0 > 0 && i0 - 1 < L && reach[i0 - 1] && mlen[i0 - 1] == 0;
  int last_start = -1;   // the last literal run that starts among this thread's positions
#pragma unroll
  for (int j = 0; j < DFL_PER; j++)
    if (kind[j] == 1 && !(j == 0 ? lit_before : kind[j - 1] == 1)) last_start = i0 + j;
  int inc_max = last_start;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc_max, d, 64);
    if (lane >= d && up > inc_max) inc_max = up;
  }
  if (lane == 63) wave_max[wave] = inc_max;
  int run_start = __shfl_up(inc_max, 1, 64);
  if (lane == 0) run_start = -1;
  __syncthreads();
  for (int w = 0; w < wave; w++)
    if (wave_max[w] > run_start) run_start = wave_max[w];
  unsigned char size[DFL_PER];
  unsigned short in_run[DFL_PER];   // a literal's index inside its run
  unsigned int sum = 0;
#pragma unroll
  for (int j = 0; j < DFL_PER; j++) {
    const int i = i0 + j;
    size[j] = 0;
    in_run[j] = 0;
    if (kind[j] == 1) {
      if (!(j == 0 ? lit_before : kind[j - 1] == 1)) run_start = i;
      in_run[j] = (unsigned short)(i - run_start);
      size[j] = (in_run[j] & 31) == 0 ? 2 : 1;
    } else if (kind[j] == 2) {
      size[j] = len16[j] <= 8 ? 2 : 3;
    }
    sum += size[j];
  }
  unsigned int inc_sum = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int up = __shfl_up(inc_sum, d, 64);
    if (lane >= d) inc_sum += up;
  }
  if (lane == 63) wave_sum[wave] = inc_sum;
  __syncthreads();
  unsigned int at = inc_sum - sum;
  for (int w = 0; w < wave; w++) at += wave_sum[w];
  if (tid == DFL_WG - 1) total_s = at + sum;

  // 5. tokens (at + size <= DFL_SLOT: the bound above)
#pragma unroll
  for (int j = 0; j < DFL_PER; j++) {
    const int i = i0 + j;
    if (kind[j] == 1) {
      if ((in_run[j] & 31) == 0) {
        int c = 1;
        while (c < 32 && i + c < L && reach[i + c] && mlen[i + c] == 0) c++;
        out[at++] = (unsigned char)(c - 1);
      }
      out[at++] = data[i];
    } else if (kind[j] == 2) {
      const unsigned int d = (unsigned int)(i - (int)cand[i] - 1), l = (unsigned int)len16[j] - 2u;
      if (l < 7u) {
        out[at++] = (unsigned char)((l << 5) | (d >> 8));
      } else {
        out[at++] = (unsigned char)((7u << 5) | (d >> 8));
        out[at++] = (unsigned char)(l - 7u);
      }
      out[at++] = (unsigned char)(d & 255u);
    }
  }
  __syncthreads();
  unsigned int total = total_s;
  if (total > (unsigned int)DFL_SLOT) total = DFL_SLOT;   // (never: the slot is the bound)
  unsigned int* dst = reinterpret_cast<unsigned int*>(slots + (size_t)blockIdx.x * DFL_SLOT);
  const unsigned int* out_w = reinterpret_cast<const unsigned int*>(out);
  for (int w = tid; w < (int)((total + 3u) >> 2); w += DFL_WG) dst[w] = out_w[w];
  if (tid == 0) chunk_bytes[blockIdx.x] = total;
}

constexpr int DFL_SCAN_WG = 1024;

__global__ __launch_bounds__(DFL_SCAN_WG) void dfl_scan_kernel(const unsigned int* __restrict__ sums, int nb,
                                                               unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long wave_tot[DFL_SCAN_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long chunk = ((long long)nb + DFL_SCAN_WG - 1) / DFL_SCAN_WG;
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
  if (tid == DFL_SCAN_WG - 1) offsets[nb] = run;   // the last thread's part ends at nb (or is empty behind it): run is the total
}

__global__ __launch_bounds__(DFL_WG) void dfl_compact_kernel(const unsigned char* __restrict__ slots, const unsigned int* __restrict__ chunk_bytes,
                                                             const unsigned long long* __restrict__ offsets, unsigned char* __restrict__ stream) {
  __shared__ unsigned int image[DFL_SLOT / 4 + 1];   // the chunk's stream plus up to three bytes of lead
  const int tid = threadIdx.x;
  unsigned int total = chunk_bytes[blockIdx.x];
  const unsigned long long room = offsets[blockIdx.x + 1] - offsets[blockIdx.x];
  if ((unsigned long long)total > room) total = (unsigned int)room;
  if (total > (unsigned int)DFL_SLOT) total = DFL_SLOT;
  unsigned char* dst = stream + offsets[blockIdx.x];
  const int shift = (int)((uintptr_t)dst & 3);
  unsigned char* img = reinterpret_cast<unsigned char*>(image);
  const unsigned int* src = reinterpret_cast<const unsigned int*>(slots + (size_t)blockIdx.x * DFL_SLOT);
  for (int w = tid; w < (int)((total + 3u) >> 2); w += DFL_WG) {   // (a slot is a whole number of words)
    const unsigned int v = src[w];
    for (int b = 0; b < 4; b++) img[shift + 4 * w + b] = (unsigned char)(v >> (8 * b));
  }
  __syncthreads();
  // image bytes [shift, span) go to dst - shift + [shift, span): word w of the image is the aligned word w behind dst - shift
  const int span = shift + (int)total, n_words = (span + 3) >> 2;
  unsigned char* g0 = dst - shift;
  for (int w = tid; w < n_words; w += DFL_WG) {
    const int lo = 4 * w, hi = lo + 4;
    if (lo >= shift && hi <= span) {
      reinterpret_cast<unsigned int*>(g0)[w] = image[w];
    } else {
      const int a = lo > shift ? lo : shift, b = hi < span ? hi : span;
      for (int c = a; c < b; c++) g0[c] = img[c];
    }
  }
}

int check_count(size_t n, const char* who) {
  if (n == 0 || n > (size_t)INT32_MAX) { set_last_error(std::string(who) + ": count out of range"); return LSR_ERR_INVALID_ARGUMENT; }
  return LSR_OK;
}

}  // namespace

int pcd_pack_records(const void* d_records, size_t n, const PcdFields& F, unsigned char* d_packed, hipStream_t stream) {
  if (int st = check_count(n, "pcd_pack_records")) return st;
  hipLaunchKernelGGL(pcd_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<const unsigned char*>(d_records), (int)n, F,
                     reinterpret_cast<unsigned int*>(d_packed));
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_field_major_image(const void* d_records, size_t n, const PcdFields& F, unsigned char* d_image, hipStream_t stream) {
  if (int st = check_count(n, "pcd_field_major_image")) return st;
  hipLaunchKernelGGL(pcd_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<const unsigned char*>(d_records), (int)n, F,
                     reinterpret_cast<unsigned int*>(d_image));
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_lzf_deflate(const unsigned char* d_image, size_t n_image, unsigned char* d_slots, unsigned int* d_chunk_bytes,
                    unsigned long long* d_chunk_offsets, hipStream_t stream) {
  if (int st = check_count(n_image, "pcd_lzf_deflate")) return st;
  const int nb = (int)dfl_chunks(n_image);
  hipLaunchKernelGGL(dfl_chunk_kernel, dim3(nb), dim3(DFL_WG), 0, stream, d_image, n_image, d_slots, d_chunk_bytes);
  LSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(dfl_scan_kernel, dim3(1), dim3(DFL_SCAN_WG), 0, stream, d_chunk_bytes, nb, d_chunk_offsets);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int pcd_lzf_compact(const unsigned char* d_slots, size_t n_image, const unsigned int* d_chunk_bytes, const unsigned long long* d_chunk_offsets,
                    unsigned char* d_stream, hipStream_t stream) {
  if (int st = check_count(n_image, "pcd_lzf_compact")) return st;
  const int nb = (int)dfl_chunks(n_image);
  hipLaunchKernelGGL(dfl_compact_kernel, dim3(nb), dim3(DFL_WG), 0, stream, d_slots, d_chunk_bytes, d_chunk_offsets, d_stream);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

}  // namespace lsr
