// Writing DATA binary and DATA binary_compressed .pcd bodies on the device (csrc/pcd_deflate.hip): records of an lsr_pc2_layout in HBM ->
// packed records, or -> the field-major image and its LZF stream, and what a handle keeps for it (lsr_format_pcd, lsr_save_pcd,
// lsr_save_map_pcd).  The stream is a pure function of the image: the image is cut into chunks of LSR_PCD_LZF_CHUNK_BYTES, each chunk
// compressed on its own by one workgroup under the rule written down in pcd_deflate.hip, and the chunks' streams concatenated.
#pragma once
#include "pcd_text.hpp"

namespace lsr {

constexpr int DFL_CHUNK = LSR_PCD_LZF_CHUNK_BYTES;
constexpr int DFL_SLOT = DFL_CHUNK + DFL_CHUNK / 32;   // the longest stream of a chunk: literal runs of 32 alone
constexpr int DFL_MAX_LEN = 264;                       // the longest reference: 2 + 7 + 255

struct PcdDeflateState {
  double deflate_ms = 0.0;                   // LSR_PCD_DEFLATE_MS
  DevBuf<unsigned char> image;               // the field-major image of the whole cloud
  DevBuf<unsigned char> slots;               // per chunk DFL_SLOT bytes: its stream, before the chunks are moved together
  DevBuf<unsigned int> chunk_bytes;          // per chunk: the length of its stream
  DevBuf<unsigned long long> chunk_offsets;  // their exclusive scan, the total behind it
  DevBuf<unsigned char> stream;              // the whole stream
};

inline size_t dfl_chunks(size_t image_bytes) { return (image_bytes + DFL_CHUNK - 1) / DFL_CHUNK; }

// n records (n <= INT32_MAX) -> n packed records of 4 * F.n_fields bytes at d_packed (4-byte aligned), the fields copied bit for bit
int pcd_pack_records(const void* d_records, size_t n, const PcdFields& F, unsigned char* d_packed, hipStream_t stream);
// n records -> the field-major image at d_image (4-byte aligned): per field, in F's order, a block of 4 n bytes
int pcd_field_major_image(const void* d_records, size_t n, const PcdFields& F, unsigned char* d_image, hipStream_t stream);
// The image's chunks compressed (d_image 4-byte aligned, n_image <= INT32_MAX): d_slots[dfl_chunks * DFL_SLOT] (4-byte aligned) the
// chunks' streams, d_chunk_bytes[dfl_chunks] their lengths, d_chunk_offsets[dfl_chunks + 1] the exclusive scan with the total last.
int pcd_lzf_deflate(const unsigned char* d_image, size_t n_image, unsigned char* d_slots, unsigned int* d_chunk_bytes,
                    unsigned long long* d_chunk_offsets, hipStream_t stream);
// The chunks' streams moved together at d_stream (any alignment; d_chunk_offsets' last entry bytes).  One writer per byte.
int pcd_lzf_compact(const unsigned char* d_slots, size_t n_image, const unsigned int* d_chunk_bytes, const unsigned long long* d_chunk_offsets,
                    unsigned char* d_stream, hipStream_t stream);

}  // namespace lsr
