// The whole map from its submaps and map.pcd: lsr_assemble_map, lsr_format_pcd_ascii, lsr_save_pcd_ascii and lsr_save_map_pcd_ascii of
// the C ABI (include/lidarslam_reg.h), and their forms with a body kind, lsr_format_pcd, lsr_save_pcd, lsr_save_map_pcd, with
// lsr_lzf_deflate.  Host-side orchestration only: staging, the launches of cloud_codec / pcd_text / pcd_deflate, the file.
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>

#include "api_internal.hpp"

using namespace lsr;

namespace {
constexpr size_t MAP_STAGE_BYTES = (size_t)64 << 20;
bool is_xyzi_layout(const lsr_pc2_layout* L) {
  return L->point_step == 32 && L->offset_x == 0 && L->offset_y == 4 && L->offset_z == 8 && L->offset_intensity == 16;
}

int pcd_check_args(const void* data, size_t n, const lsr_pc2_layout* layout, PcdFields* F) {
  if (!data) { set_last_error("data: null record pointer"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_layout(layout);
  if (st) return st;
  if (n == 0) { set_last_error("n_points: an empty cloud has no PCD file"); return LSR_ERR_INVALID_ARGUMENT; }   // PCL refuses it too
  if ((st = arg_error(check_records(data, n, MAP_RECORD_LIMIT, true, "data")))) return st;
  F->step = (int)layout->point_step;
  F->n_fields = layout->offset_intensity >= 0 ? 4 : 3;
  F->off[0] = (int)layout->offset_x; F->off[1] = (int)layout->offset_y; F->off[2] = (int)layout->offset_z;
  F->off[3] = layout->offset_intensity >= 0 ? layout->offset_intensity : 0;
  return LSR_OK;
}
int pcd_io_error(const char* what, const char* path) {
  set_last_error(std::string(what) + " " + path + ": " + std::strerror(errno));
  return LSR_ERR_IO;
}
// the file being written: closed and removed unless the call gets as far as commit() (a device node such as /dev/null is only closed)
struct PcdFile {
  FILE* f = nullptr;
  const char* path = nullptr;
  bool regular = false;
  ~PcdFile() {
    if (!f) return;
    (void)std::fclose(f);
    if (regular) (void)std::remove(path);
  }
  int commit() {
    FILE* g = f;
    f = nullptr;
    if (std::fclose(g) == 0) return 0;
    const int e = errno;
    if (regular) (void)std::remove(path);
    errno = e;
    return -1;
  }
  int open(const char* p) {
    path = p;
    f = std::fopen(p, "wb");
    if (!f) return pcd_io_error("cannot open", p);
    struct stat sb;
    regular = fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode);
    return LSR_OK;
  }
};

int pcd_check_kind(int data_kind) {
  if (data_kind == LSR_PCD_ASCII || data_kind == LSR_PCD_BINARY || data_kind == LSR_PCD_BINARY_COMPRESSED) return LSR_OK;
  set_last_error("data_kind: not LSR_PCD_ASCII, LSR_PCD_BINARY or LSR_PCD_BINARY_COMPRESSED");
  return LSR_ERR_INVALID_ARGUMENT;
}

// The records' field-major image compressed in HBM on the object's stream: gather, chunk compressor, scan; the total read back
// (*c_size; the stream is idle then); with `compact` the chunks' streams moved together into D.stream (enqueued, not waited for: the
// caller brackets it with its own copy).  *ms: the launches' hipEvent time, when profiling (the compaction's bracket closes at EV_W1).
int pcd_deflate_image(lsr_handle h, size_t u_size, bool compact, size_t* c_size, double* ms);
int pcd_deflate_records(lsr_handle h, const void* d_records, size_t n, const PcdFields& F, bool compact, size_t* c_size, double* ms) {
  PcdDeflateState& D = h->pcd_deflate;
  const size_t u_size = n * 4 * (size_t)F.n_fields;
  int st;
  if ((st = h->pcd.ensure_events()) || (st = D.image.reserve(u_size))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(h->pcd.ev[0][PcdState::EV_L0], h->stream));
  if ((st = pcd_field_major_image(d_records, n, F, D.image.p, h->stream))) return st;
  return pcd_deflate_image(h, u_size, compact, c_size, ms);
}
// the same from the image, u_size bytes in D.image (the caller has opened the bracket at EV_L0)
int pcd_deflate_image(lsr_handle h, size_t u_size, bool compact, size_t* c_size, double* ms) {
  PcdState& S = h->pcd;
  PcdDeflateState& D = h->pcd_deflate;
  const size_t nb = dfl_chunks(u_size);
  int st;
  if ((st = S.totals.reserve(2)) || (st = D.slots.reserve(nb * DFL_SLOT)) || (st = D.chunk_bytes.reserve(nb)) ||
      (st = D.chunk_offsets.reserve(nb + 1)))
    return st;
  hipEvent_t* ev = S.ev[0];
  if ((st = pcd_lzf_deflate(D.image.p, u_size, D.slots.p, D.chunk_bytes.p, D.chunk_offsets.p, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_L1], h->stream));
  LSR_HIP(hipMemcpyAsync(S.totals.p, D.chunk_offsets.p + nb, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  const unsigned long long total = S.totals.p[0];
  if (h->profile && (st = add_ms(ev[PcdState::EV_L0], ev[PcdState::EV_L1], ms))) return st;
  if (total > (unsigned long long)INT32_MAX) { set_last_error("the compressed stream has more than 2^31 - 1 bytes"); return LSR_ERR_INDEX_OVERFLOW; }
  if (total == 0 || total > (unsigned long long)nb * DFL_SLOT) { set_last_error("the compressed stream is longer than its bound"); return LSR_ERR_HIP; }
  *c_size = (size_t)total;
  if (!compact) return LSR_OK;
  if ((st = D.stream.reserve((size_t)total))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_W0], h->stream));
  if ((st = pcd_lzf_compact(D.slots.p, u_size, D.chunk_bytes.p, D.chunk_offsets.p, D.stream.p, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_W1], h->stream));
  return LSR_OK;
}

// header, and for a compressed body the two size words behind it; returns the length
size_t pcd_binary_header(size_t n, const PcdFields& F, int data_kind, size_t c_size, char* out /* PCD_MAX_HEADER_BYTES + 8 */) {
  size_t len = (size_t)pcd_header_text(n, F.n_fields == 4, out, data_kind == LSR_PCD_BINARY ? "binary" : "binary_compressed");
  if (data_kind == LSR_PCD_BINARY_COMPRESSED) {
    const uint32_t words[2] = {(uint32_t)c_size, (uint32_t)(n * 4 * (size_t)F.n_fields)};
    for (int w = 0; w < 2; w++)
      for (int b = 0; b < 4; b++) out[len++] = (char)(unsigned char)(words[w] >> (8 * b));   // little endian
  }
  return len;
}

int pcd_check_image_size(size_t n, const PcdFields& F, int data_kind) {
  if (data_kind == LSR_PCD_BINARY_COMPRESSED && n * 4 * (size_t)F.n_fields > (size_t)INT32_MAX) {
    set_last_error("n_points: the uncompressed image has more than 2^31 - 1 bytes");
    return LSR_ERR_INDEX_OVERFLOW;
  }
  return LSR_OK;
}
}  // namespace

extern "C" {

// ---- N5: the whole map from its submaps ---------------------------------------------------------
// ScanMatcherComponent::publishMap (scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment
// (graph_based_slam_component.cpp:321-368).  One launch per piece: with every buffer on the device the whole map is one piece; a host
// input or output is staged MAP_STAGE_BYTES at a time (a long submap is cut: a table slot is a run of records with a pose, not a submap).
int lsr_assemble_map(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                     const double* poses16, void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device,
                     size_t* first_record, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!submaps || num_submaps <= 0 || !n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_layout(in_layout, "in_layout");
  if (st) return st;
  if ((st = check_out_layout(out_layout))) return st;
  const size_t in_step = in_layout->point_step, out_step = out_layout->point_step;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  size_t total = 0;
  bool aligned16 = true;
  for (int i = 0; i < num_submaps; i++) {
    const lsr_submap& s = submaps[i];
    if (s.n_points == 0) continue;
    if ((st = arg_error(check_records(s.cloud, s.n_points, MAP_RECORD_LIMIT, true, "submaps[].cloud")))) return st;
    if ((uintptr_t)s.cloud & 15) aligned16 = false;
    if ((st = arg_error(check_record_count(total += s.n_points, MAP_RECORD_LIMIT, "submaps[] (the whole map)")))) return st;
  }
  if (total > capacity_points) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = arg_error(check_records(out_data, total, MAP_RECORD_LIMIT, true, "out_data")))) return st;
  if (in_host == out_host)
    for (int i = 0; i < num_submaps; i++)
      if (ranges_overlap(out_data, total * out_step, submaps[i].cloud, submaps[i].n_points * in_step)) {
        set_last_error("the output range overlaps an input cloud");
        return LSR_ERR_INVALID_ARGUMENT;
      }
  auto finish = [&]() {
    if (first_record) {
      size_t off = 0;
      for (int i = 0; i < num_submaps; i++) { first_record[i] = off; off += submaps[i].n_points; }
      first_record[num_submaps] = off;
    }
    *n_out = total;
    return LSR_OK;
  };
  if (total == 0) return finish();

  // poses: tf2::fromMsg -> Affine3d -> .cast<float>() (publishMap :538-542) or the optimiser's estimates (:329-342), cast the same way
  std::vector<float> T((size_t)num_submaps * 16);
  for (int i = 0; i < num_submaps; i++) {
    double M[16];
    if (poses16) std::memcpy(M, poses16 + 16 * (size_t)i, sizeof(M)); else submap_pose_matrix(submaps[i], M);
    for (int k = 0; k < 16; k++) T[16 * (size_t)i + k] = (float)M[k];
  }
  // the wide form needs every base pointer on a 16-byte boundary; staged records are (32-byte records, back to back in a hipMalloc'ed buffer)
  const bool wide = is_xyzi_layout(in_layout) && is_xyzi_layout(out_layout) && (in_host || aligned16) && (out_host || ((uintptr_t)out_data & 15) == 0);
  MapLayouts L;
  L.in_step = in_layout->point_step; L.in_x = in_layout->offset_x; L.in_y = in_layout->offset_y; L.in_z = in_layout->offset_z;
  L.in_intensity = in_layout->offset_intensity;
  L.out_step = out_layout->point_step; L.out_x = out_layout->offset_x; L.out_y = out_layout->offset_y; L.out_z = out_layout->offset_z;
  L.out_intensity = out_layout->offset_intensity;

  const size_t piece_cap = (in_host || out_host) ? std::max<size_t>(1, MAP_STAGE_BYTES / std::max(in_step, out_step)) : total;
  if (in_host && (st = h->staging.reserve(std::min(total, piece_cap) * in_step))) return st;
  if (out_host && (st = h->map_out.reserve(std::min(total, piece_cap) * out_step))) return st;
  // whatever was enqueued has finished before the call returns: the table, the staging buffers and the caller's buffers are free again
  StreamDrain drain{h->stream};
  std::vector<MapSlot> slots;
  double map_ms = 0.0;
  size_t done = 0, at = 0;   // records written so far; position inside submap `i`
  int i = 0;
  while (done < total) {
    slots.clear();
    size_t piece = 0;
    int n_slices = 0;
    while (i < num_submaps && piece < piece_cap) {
      const size_t left = submaps[i].n_points - at;
      if (left == 0) { i++; at = 0; continue; }
      const size_t take = std::min(left, piece_cap - piece);
      const unsigned char* src = static_cast<const unsigned char*>(submaps[i].cloud) + at * in_step;
      MapSlot S;
      const void* d_src = nullptr;
      if ((st = stage_in_at(h, src, take * in_step, !in_host, h->stream, piece * in_step, &d_src))) return st;
      S.records = static_cast<const unsigned char*>(d_src);
      S.first_out = (long long)((out_host ? 0 : done) + piece);
      S.count = (int)take;
      S.first_slice = n_slices;
      std::memcpy(S.T16, T.data() + 16 * (size_t)i, sizeof(S.T16));
      slots.push_back(S);
      n_slices += (int)((take + MAP_SLICE - 1) / MAP_SLICE);
      piece += take;
      at += take;
    }
    if ((st = h->h_map_slots.reserve(slots.size()))) return st;
    if ((st = h->d_map_slots.reserve(slots.size()))) return st;
    std::memcpy(h->h_map_slots.p, slots.data(), sizeof(MapSlot) * slots.size());
    LSR_HIP(hipMemcpyAsync(h->d_map_slots.p, h->h_map_slots.p, sizeof(MapSlot) * slots.size(), hipMemcpyHostToDevice, h->stream));
    void* d_out = out_host ? static_cast<void*>(h->map_out.p) : out_data;
    if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));   // LSR_PROFILE: the launch alone, staging copies outside the bracket
    if ((st = assemble_map(h->d_map_slots.p, (int)slots.size(), n_slices, wide, L, d_out, h->stream))) return st;
    if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
    if (out_host)
      LSR_HIP(hipMemcpyAsync(static_cast<unsigned char*>(out_data) + done * out_step, h->map_out.p, piece * out_step, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));   // the pinned table and the staging buffers are reused by the next piece
    if (h->profile) {
      float ms = 0.f;
      LSR_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
      map_ms += ms;
    }
    done += piece;
  }
  h->map_form = wide ? 1 : 2;
  h->map_ms = map_ms;
  return finish();
}

// ---- N7: map.pcd -------------------------------------------------------------------------------
// pcl::io::savePCDFileASCII("map.pcd", *map_ptr) (graph_based_slam_component.cpp:369): the text is formatted on the device (pcd_text.hip).
int lsr_format_pcd_ascii(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, void* out_text,
                         size_t capacity_bytes, int out_on_device, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!n_bytes) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  PcdFields F;
  int st = pcd_check_args(data, n_points, layout, &F);
  if (st) return st;
  PcdState& S = h->pcd;
  const size_t nb = pcd_blocks(n_points);
  if ((st = S.ensure_events()) || (st = S.block_sums[0].reserve(nb)) || (st = S.offsets[0].reserve(nb + 1)) || (st = S.totals.reserve(2)) ||
      (st = S.header.reserve(PCD_MAX_HEADER_BYTES)))
    return st;
  // whatever was enqueued has finished before the call returns: the staging buffer and the caller's buffers are free again
  StreamDrain drain{h->stream};
  const void* d = nullptr;
  if ((st = stage_in(h, data, n_points * F.step, on_device != 0, h->stream, &d))) return st;
  hipEvent_t* ev = S.ev[0];
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_L0], h->stream));
  if ((st = pcd_text_lengths(d, n_points, F, S.block_sums[0].p, S.offsets[0].p, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_L1], h->stream));
  LSR_HIP(hipMemcpyAsync(S.totals.p, S.offsets[0].p + nb, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  const size_t body = (size_t)S.totals.p[0];
  char header[PCD_MAX_HEADER_BYTES];
  const size_t header_bytes = (size_t)pcd_header_text(n_points, F.n_fields == 4, header);
  const size_t size = header_bytes + body;
  double ms = 0.0;
  if (h->profile && (st = add_ms(ev[PcdState::EV_L0], ev[PcdState::EV_L1], &ms))) return st;
  if (!out_text) {
    S.format_ms = ms;
    *n_bytes = size;
    return LSR_OK;
  }
  if (capacity_bytes < size) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  unsigned char* d_text = nullptr;
  if (out_on_device) {
    std::memcpy(S.header.p, header, header_bytes);
    LSR_HIP(hipMemcpyAsync(out_text, S.header.p, header_bytes, hipMemcpyHostToDevice, h->stream));
    d_text = static_cast<unsigned char*>(out_text) + header_bytes;
  } else {
    if ((st = S.text.reserve(body))) return st;
    d_text = S.text.p;
  }
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_W0], h->stream));
  if ((st = pcd_text_write(d, n_points, F, S.offsets[0].p, d_text, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(ev[PcdState::EV_W1], h->stream));
  if (!out_on_device)
    LSR_HIP(hipMemcpyAsync(static_cast<unsigned char*>(out_text) + header_bytes, S.text.p, body, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (!out_on_device) std::memcpy(out_text, header, header_bytes);
  if (h->profile && (st = add_ms(ev[PcdState::EV_W0], ev[PcdState::EV_W1], &ms))) return st;
  S.format_ms = ms;
  *n_bytes = size;
  return LSR_OK;
}

int lsr_save_pcd_ascii(lsr_handle h, const char* path, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device,
                       size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_bytes) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  PcdFields F;
  int st = pcd_check_args(data, n_points, layout, &F);
  if (st) return st;
  PcdState& S = h->pcd;
  const size_t P = (size_t)S.piece_records, n_pieces = (n_points + P - 1) / P, p_max = std::min(P, n_points);
  const size_t nb_max = pcd_blocks(p_max), text_max = p_max * PCD_MAX_LINE_BYTES;
  if ((st = S.ensure_events()) || (st = S.totals.reserve(2)) || (st = S.text.reserve(text_max))) return st;
  for (int par = 0; par < 2; par++)
    if ((st = S.block_sums[par].reserve(nb_max)) || (st = S.offsets[par].reserve(nb_max + 1)) || (st = S.pin[par].reserve(text_max))) return st;
  const bool in_host = on_device == 0;
  if (in_host && (st = h->staging.reserve(2 * p_max * F.step))) return st;

  PcdFile file;
  file.path = path;
  file.f = std::fopen(path, "wb");
  if (!file.f) return pcd_io_error("cannot open", path);
  {
    struct stat sb;
    file.regular = fstat(fileno(file.f), &sb) == 0 && S_ISREG(sb.st_mode);
  }
  StreamDrain drain{h->stream};   // (destroyed before `file`: nothing is in flight when the file is closed)
  char header[PCD_MAX_HEADER_BYTES];
  const size_t header_bytes = (size_t)pcd_header_text(n_points, F.n_fields == 4, header);
  if (std::fwrite(header, 1, header_bytes, file.f) != header_bytes) return pcd_io_error("short write to", path);
  size_t written = header_bytes;
  double ms = 0.0;

  const void* d_piece[2] = {nullptr, nullptr};
  size_t count[2] = {0, 0}, bytes[2] = {0, 0};
  // stream order: len(k + 1) | write(k) copy(k) | len(k + 2) | write(k + 1) ... — the host learns a piece's size one piece ahead of
  // laying it out, and writes piece k - 1 to the file while the device works on the three steps in front of it
  auto enqueue_lengths = [&](size_t k) -> int {
    const int par = (int)(k & 1);
    const size_t first = k * P, cnt = std::min(P, n_points - first);
    const void* src = nullptr;   // host pieces alternate between the two halves of the staging buffer
    int e = stage_in_at(h, static_cast<const unsigned char*>(data) + first * F.step, cnt * F.step, !in_host, h->stream,
                        (size_t)par * p_max * F.step, &src);
    if (e) return e;
    d_piece[par] = src;
    count[par] = cnt;
    if (h->profile) LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_L0], h->stream));
    e = pcd_text_lengths(src, cnt, F, S.block_sums[par].p, S.offsets[par].p, h->stream);
    if (e) return e;
    if (h->profile) LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_L1], h->stream));
    LSR_HIP(hipMemcpyAsync(S.totals.p + par, S.offsets[par].p + pcd_blocks(cnt), sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_LEN], h->stream));
    return LSR_OK;
  };
  auto flush = [&](size_t k) -> int {
    const int par = (int)(k & 1);
    LSR_HIP(hipEventSynchronize(S.ev[par][PcdState::EV_DONE]));
    if (h->profile) {
      int e = add_ms(S.ev[par][PcdState::EV_W0], S.ev[par][PcdState::EV_W1], &ms);
      if (e) return e;
    }
    if (std::fwrite(S.pin[par].p, 1, bytes[par], file.f) != bytes[par]) return pcd_io_error("short write to", path);
    written += bytes[par];
    return LSR_OK;
  };

  if ((st = enqueue_lengths(0))) return st;
  for (size_t k = 0; k < n_pieces; k++) {
    const int par = (int)(k & 1);
    LSR_HIP(hipEventSynchronize(S.ev[par][PcdState::EV_LEN]));
    bytes[par] = (size_t)S.totals.p[par];
    if (bytes[par] > count[par] * PCD_MAX_LINE_BYTES) { set_last_error("a piece's text is longer than its bound"); return LSR_ERR_HIP; }
    if (h->profile && (st = add_ms(S.ev[par][PcdState::EV_L0], S.ev[par][PcdState::EV_L1], &ms))) return st;
    if (k + 1 < n_pieces && (st = enqueue_lengths(k + 1))) return st;
    if (h->profile) LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_W0], h->stream));
    if ((st = pcd_text_write(d_piece[par], count[par], F, S.offsets[par].p, S.text.p, h->stream))) return st;
    if (h->profile) LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_W1], h->stream));
    LSR_HIP(hipMemcpyAsync(S.pin[par].p, S.text.p, bytes[par], hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_DONE], h->stream));
    if (k >= 1 && (st = flush(k - 1))) return st;
  }
  if ((st = flush(n_pieces - 1))) return st;
  if (file.commit() != 0) return pcd_io_error("cannot close", path);
  S.format_ms = ms;
  *n_bytes = written;
  return LSR_OK;
}

int lsr_save_map_pcd_ascii(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                           int on_device, const double* poses16, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_bytes || !submaps || num_submaps <= 0) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  int st;
  for (int i = 0; i < num_submaps; i++)   // (the size of the map buffer; lsr_assemble_map below checks the clouds themselves)
    if ((st = arg_error(check_record_count(submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[].n_points"))) ||
        (st = arg_error(check_record_count(total += submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[] (the whole map)"))))
      return st;
  if (total == 0) { set_last_error("submaps[]: an empty map has no PCD file"); return LSR_ERR_INVALID_ARGUMENT; }
  static const lsr_pc2_layout xyzi = {32, 0, 4, 8, 16};   // pcl::PointXYZI, what map_ptr holds
  if ((st = h->pcd.map.reserve(total * xyzi.point_step))) return st;
  size_t n = 0;
  if ((st = lsr_assemble_map(h, submaps, num_submaps, in_layout, on_device, poses16, h->pcd.map.p, total, &xyzi, 1, nullptr, &n))) return st;
  return lsr_save_pcd_ascii(h, path, h->pcd.map.p, n, &xyzi, 1, n_bytes);
}

// ---- map.pcd as DATA binary / DATA binary_compressed (csrc/pcd_deflate.hip) ----------------------
int lsr_format_pcd(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, int data_kind,
                   void* out_image, size_t capacity_bytes, int out_on_device, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!n_bytes) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = pcd_check_kind(data_kind);
  if (st) return st;
  if (data_kind == LSR_PCD_ASCII) {
    if ((st = lsr_format_pcd_ascii(h, data, n_points, layout, on_device, out_image, capacity_bytes, out_on_device, n_bytes))) return st;
    h->pcd_deflate.deflate_ms = 0.0;
    return LSR_OK;
  }
  PcdFields F;
  if ((st = pcd_check_args(data, n_points, layout, &F)) || (st = pcd_check_image_size(n_points, F, data_kind))) return st;
  PcdState& S = h->pcd;
  PcdDeflateState& D = h->pcd_deflate;
  const bool compressed = data_kind == LSR_PCD_BINARY_COMPRESSED;
  const size_t rec_bytes = 4 * (size_t)F.n_fields;
  if ((st = S.ensure_events()) || (st = S.header.reserve(PCD_MAX_HEADER_BYTES + 8))) return st;
  // whatever was enqueued has finished before the call returns: the staging buffer and the caller's buffers are free again
  StreamDrain drain{h->stream};
  double ms = 0.0;
  size_t body = n_points * rec_bytes;   // behind the header (and the size words)
  const void* d = nullptr;
  if (compressed) {
    if ((st = stage_in(h, data, n_points * F.step, on_device != 0, h->stream, &d)) ||
        (st = pcd_deflate_records(h, d, n_points, F, out_image != nullptr, &body, &ms)))
      return st;
  }
  char header[PCD_MAX_HEADER_BYTES + 8];
  const size_t header_bytes = pcd_binary_header(n_points, F, data_kind, body, header);
  const size_t size = header_bytes + body;
  if (!out_image) {
    D.deflate_ms = ms;
    *n_bytes = size;
    return LSR_OK;
  }
  if (capacity_bytes < size) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  const unsigned char* d_body = D.stream.p;
  if (!compressed) {
    if ((st = S.text.reserve(body)) || (st = stage_in(h, data, n_points * F.step, on_device != 0, h->stream, &d)) ||
        (st = pcd_pack_records(d, n_points, F, S.text.p, h->stream)))
      return st;
    d_body = S.text.p;
  }
  unsigned char* out = static_cast<unsigned char*>(out_image);
  if (out_on_device) {
    std::memcpy(S.header.p, header, header_bytes);
    LSR_HIP(hipMemcpyAsync(out, S.header.p, header_bytes, hipMemcpyHostToDevice, h->stream));
    LSR_HIP(hipMemcpyAsync(out + header_bytes, d_body, body, hipMemcpyDeviceToDevice, h->stream));
  } else {
    LSR_HIP(hipMemcpyAsync(out + header_bytes, d_body, body, hipMemcpyDeviceToHost, h->stream));
  }
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (!out_on_device) std::memcpy(out, header, header_bytes);
  if (compressed && h->profile && (st = add_ms(S.ev[0][PcdState::EV_W0], S.ev[0][PcdState::EV_W1], &ms))) return st;
  D.deflate_ms = ms;
  *n_bytes = size;
  return LSR_OK;
}

int lsr_save_pcd(lsr_handle h, const char* path, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, int data_kind,
                 size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_bytes) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = pcd_check_kind(data_kind);
  if (st) return st;
  if (data_kind == LSR_PCD_ASCII) {
    if ((st = lsr_save_pcd_ascii(h, path, data, n_points, layout, on_device, n_bytes))) return st;
    h->pcd_deflate.deflate_ms = 0.0;
    return LSR_OK;
  }
  PcdFields F;
  if ((st = pcd_check_args(data, n_points, layout, &F)) || (st = pcd_check_image_size(n_points, F, data_kind))) return st;
  PcdState& S = h->pcd;
  PcdDeflateState& D = h->pcd_deflate;
  const bool compressed = data_kind == LSR_PCD_BINARY_COMPRESSED, in_host = on_device == 0;
  const size_t rec_bytes = 4 * (size_t)F.n_fields;
  const size_t P = (size_t)S.piece_records, p_max = std::min(P, n_points), piece_bytes = p_max * rec_bytes;
  if ((st = S.ensure_events())) return st;
  for (int par = 0; par < 2; par++)
    if ((st = S.pin[par].reserve(piece_bytes))) return st;
  if (compressed) {
    if (in_host && (st = h->staging.reserve(n_points * F.step))) return st;
  } else {
    if ((st = S.text.reserve(piece_bytes)) || (in_host && (st = h->staging.reserve(2 * p_max * F.step)))) return st;
  }

  PcdFile file;
  if ((st = file.open(path))) return st;
  StreamDrain drain{h->stream};   // (destroyed before `file`: nothing is in flight when the file is closed)
  double ms = 0.0;
  size_t body = n_points * rec_bytes;
  if (compressed) {
    const void* d = nullptr;
    if ((st = stage_in_at(h, data, n_points * F.step, !in_host, h->stream, 0, &d)) || (st = pcd_deflate_records(h, d, n_points, F, true, &body, &ms)))
      return st;
  }
  char header[PCD_MAX_HEADER_BYTES + 8];
  const size_t header_bytes = pcd_binary_header(n_points, F, data_kind, body, header);
  if (std::fwrite(header, 1, header_bytes, file.f) != header_bytes) return pcd_io_error("short write to", path);
  size_t written = header_bytes;

  // piece k + 1 is packed (binary) and copied into one pinned buffer while the calling thread writes piece k from the other
  const size_t n_pieces = (body + piece_bytes - 1) / piece_bytes;
  size_t bytes[2] = {0, 0};
  auto enqueue = [&](size_t k) -> int {
    const int par = (int)(k & 1);
    const size_t first = k * piece_bytes;
    bytes[par] = std::min(piece_bytes, body - first);
    const unsigned char* d_piece = nullptr;
    if (compressed) {
      d_piece = D.stream.p + first;
    } else {
      const size_t rec0 = k * p_max, cnt = bytes[par] / rec_bytes;
      const void* src = nullptr;   // host pieces alternate between the two halves of the staging buffer
      int e = stage_in_at(h, static_cast<const unsigned char*>(data) + rec0 * F.step, cnt * F.step, !in_host, h->stream,
                          (size_t)par * p_max * F.step, &src);
      if (e || (e = pcd_pack_records(src, cnt, F, S.text.p, h->stream))) return e;
      d_piece = S.text.p;
    }
    LSR_HIP(hipMemcpyAsync(S.pin[par].p, d_piece, bytes[par], hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipEventRecord(S.ev[par][PcdState::EV_DONE], h->stream));
    return LSR_OK;
  };
  if ((st = enqueue(0))) return st;
  for (size_t k = 0; k < n_pieces; k++) {
    const int par = (int)(k & 1);
    if (k + 1 < n_pieces && (st = enqueue(k + 1))) return st;
    LSR_HIP(hipEventSynchronize(S.ev[par][PcdState::EV_DONE]));
    if (std::fwrite(S.pin[par].p, 1, bytes[par], file.f) != bytes[par]) return pcd_io_error("short write to", path);
    written += bytes[par];
  }
  if (compressed && h->profile && (st = add_ms(S.ev[0][PcdState::EV_W0], S.ev[0][PcdState::EV_W1], &ms))) return st;
  if (file.commit() != 0) return pcd_io_error("cannot close", path);
  D.deflate_ms = ms;
  *n_bytes = written;
  return LSR_OK;
}

int lsr_save_map_pcd(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                     int on_device, const double* poses16, int data_kind, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_bytes || !submaps || num_submaps <= 0) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = pcd_check_kind(data_kind);
  if (st) return st;
  if (data_kind == LSR_PCD_ASCII) {
    if ((st = lsr_save_map_pcd_ascii(h, path, submaps, num_submaps, in_layout, on_device, poses16, n_bytes))) return st;
    h->pcd_deflate.deflate_ms = 0.0;
    return LSR_OK;
  }
  size_t total = 0;
  for (int i = 0; i < num_submaps; i++)   // (the size of the map buffer; lsr_assemble_map below checks the clouds themselves)
    if ((st = arg_error(check_record_count(submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[].n_points"))) ||
        (st = arg_error(check_record_count(total += submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[] (the whole map)"))))
      return st;
  if (total == 0) { set_last_error("submaps[]: an empty map has no PCD file"); return LSR_ERR_INVALID_ARGUMENT; }
  static const lsr_pc2_layout xyzi = {32, 0, 4, 8, 16};   // pcl::PointXYZI, what map_ptr holds
  if ((st = h->pcd.map.reserve(total * xyzi.point_step))) return st;
  size_t n = 0;
  if ((st = lsr_assemble_map(h, submaps, num_submaps, in_layout, on_device, poses16, h->pcd.map.p, total, &xyzi, 1, nullptr, &n))) return st;
  return lsr_save_pcd(h, path, h->pcd.map.p, n, &xyzi, 1, data_kind, n_bytes);
}

int lsr_lzf_deflate(lsr_handle h, const void* image, size_t n_image, int on_device, void* out_stream, size_t capacity_bytes,
                    int out_on_device, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!image || !n_bytes) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (n_image == 0) { set_last_error("n_image: an empty image has no stream"); return LSR_ERR_INVALID_ARGUMENT; }
  if (n_image > (size_t)INT32_MAX) { set_last_error("n_image: more than 2^31 - 1 bytes"); return LSR_ERR_INDEX_OVERFLOW; }
  PcdDeflateState& D = h->pcd_deflate;
  int st;
  if ((st = h->pcd.ensure_events()) || (st = D.image.reserve(n_image))) return st;
  StreamDrain drain{h->stream};
  // (the compressor reads whole words of its own aligned copy: the caller's image may lie anywhere)
  LSR_HIP(hipMemcpyAsync(D.image.p, image, n_image, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  if (h->profile) LSR_HIP(hipEventRecord(h->pcd.ev[0][PcdState::EV_L0], h->stream));
  double ms = 0.0;
  size_t c_size = 0;
  if ((st = pcd_deflate_image(h, n_image, out_stream != nullptr, &c_size, &ms))) return st;
  if (out_stream) {
    if (capacity_bytes < c_size) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
    LSR_HIP(hipMemcpyAsync(out_stream, D.stream.p, c_size, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));
    if (h->profile && (st = add_ms(h->pcd.ev[0][PcdState::EV_W0], h->pcd.ev[0][PcdState::EV_W1], &ms))) return st;
  }
  D.deflate_ms = ms;
  *n_bytes = c_size;
  return LSR_OK;
}

}  // extern "C"
