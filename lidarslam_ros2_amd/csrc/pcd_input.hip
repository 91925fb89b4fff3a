// Reading .pcd files: lsr_parse_pcd_header, lsr_decode_pcd, lsr_load_pcd and lsr_set_input_target_pcd of the C ABI
// (include/lidarslam_reg.h).  Host-side orchestration only: the header, the pieces, the launches of pcd_read and pcd_lzf, the file, the
// two size words of a compressed body (the host reads nothing else of it), and the C library's strtof for the tokens the device left
// unresolved.
#include <sys/types.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "api_internal.hpp"

using namespace lsr;

namespace {

int pcdr_io_error(const char* what, const char* path) {
  set_last_error(std::string(what) + " " + path + ": " + (errno ? std::strerror(errno) : "unexpected end of file"));
  return LSR_ERR_IO;
}

struct PcdInFile {
  FILE* f = nullptr;
  ~PcdInFile() { if (f) (void)std::fclose(f); }
};

// one decode or load: the records of the whole file gather in the object's own buffer and are copied out at the end
struct PcdReadJob {
  lsr_handle h;
  PcdHeader H;
  PcdAsciiPlan ap;
  PcdBinaryPlan bp;
  size_t n_points = 0, step = 0, done = 0;
  double ms = 0.0, inflate_ms = 0.0;
  unsigned int unresolved_seen = 0;
  // the piece in flight
  size_t keep = 0, text_bytes = 0;
  const unsigned char* d_text = nullptr;
  bool parse_enqueued = false;
  std::vector<unsigned char> h_flags, h_records, h_text;
  std::vector<unsigned int> h_starts;
};

int job_begin(PcdReadJob& J, lsr_handle h, const lsr_pc2_layout* out) {
  J.h = h;
  J.n_points = (size_t)J.H.info.n_points;
  J.step = out->point_step;
  PcdOutFields O;
  O.step = (int)out->point_step;
  O.off[0] = (int)out->offset_x; O.off[1] = (int)out->offset_y; O.off[2] = (int)out->offset_z;
  O.off[3] = (out->offset_intensity >= 0 && J.H.info.has_intensity) ? out->offset_intensity : -1;   // no intensity in the file: +0
  for (int k = 0; k < 4; k++) { J.ap.tok[k] = J.H.tok[k]; J.bp.src[k] = J.H.src[k]; }
  if (out->offset_intensity < 0) { J.ap.tok[3] = -1; J.bp.src[3] = -1; }   // dropped: its token is not even parsed
  J.ap.n_tokens = J.H.n_tokens;
  J.ap.out = O;
  J.bp.rec_bytes = J.H.info.point_step;
  J.bp.out = O;
  PcdReadState& S = h->pcd_read;
  int st;
  if ((st = S.ensure_events()) || (st = S.records.reserve(J.n_points * J.step)) || (st = S.flags.reserve(J.n_points)) || (st = S.status.reserve(1)) ||
      (st = S.h_status.reserve(1)) || (st = S.h_total.reserve(1)))
    return st;
  S.h_status.p[0].first_error = PCDR_NO_ERROR;
  S.h_status.p[0].unresolved = 0;
  S.h_status.p[0].pad = 0;
  LSR_HIP(hipMemcpyAsync(S.status.p, S.h_status.p, sizeof(PcdReadStatus), hipMemcpyHostToDevice, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));   // h_status is written by the first piece's read-back
  return LSR_OK;
}

// An ASCII piece, first half: the text (in HBM, entered in state 0) cut into lines; the launches of the parse enqueued behind it.  Between
// this and ascii_piece_finish the calling thread is free (lsr_load_pcd reads the next piece).
int ascii_piece_launch(PcdReadJob& J, const unsigned char* d_text, size_t n_bytes) {
  lsr_handle h = J.h;
  PcdReadState& S = h->pcd_read;
  J.keep = 0;
  J.d_text = d_text;
  J.text_bytes = n_bytes;
  J.parse_enqueued = false;
  if (n_bytes == 0 || J.done >= J.n_points) return LSR_OK;
  const size_t nb = pcdr_blocks(d_text, n_bytes);
  int st;
  if ((st = S.wg_runs.reserve(nb)) || (st = S.first_slot.reserve(nb + 1)) || (st = S.entry_state.reserve(nb))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_L0], h->stream));
  if ((st = pcd_read_lines(d_text, n_bytes, S.wg_runs.p, S.first_slot.p, S.entry_state.p, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_L1], h->stream));
  LSR_HIP(hipMemcpyAsync(S.h_total.p, S.first_slot.p + nb, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (h->profile && (st = add_ms(S.ev[PcdReadState::EV_L0], S.ev[PcdReadState::EV_L1], &J.ms))) return st;
  J.keep = (size_t)std::min<unsigned long long>(S.h_total.p[0], J.n_points - J.done);
  if (J.keep == 0) return LSR_OK;
  if ((st = S.line_start.reserve(J.keep))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_P0], h->stream));
  if ((st = pcd_read_index(d_text, n_bytes, S.first_slot.p, S.entry_state.p, J.keep, S.line_start.p, h->stream))) return st;
  if ((st = pcd_read_parse(d_text, n_bytes, S.line_start.p, J.keep, J.ap, S.records.p + J.done * J.step, S.flags.p + J.done, S.status.p, h->stream)))
    return st;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[PcdReadState::EV_P1], h->stream));
  LSR_HIP(hipMemcpyAsync(S.h_status.p, S.status.p, sizeof(PcdReadStatus), hipMemcpyDeviceToHost, h->stream));
  J.parse_enqueued = true;
  return LSR_OK;
}

// token `want` of the line at text[p ..): its text, NUL-terminated, for the C library
bool host_token(const unsigned char* text, size_t n, size_t p, int want, std::string* out) {
  size_t j = p;
  for (int t = 0;; t++) {
    while (j < n && pcd_is_blank(text[j])) j++;
    if (j >= n || text[j] == '\n') return false;
    const size_t s = j;
    while (j < n && !pcd_is_blank(text[j]) && text[j] != '\n') j++;
    if (t == want) { out->assign(reinterpret_cast<const char*>(text + s), j - s); return true; }
  }
}

// Second half: the piece's errors, and its unresolved tokens settled by strtof on the host's copy of the text (host_text: the piece's
// bytes in host memory, or null: they are fetched from the device).  file_offset: of the text's first byte, for the messages.
int ascii_piece_finish(PcdReadJob& J, const unsigned char* host_text, unsigned long long file_offset) {
  lsr_handle h = J.h;
  PcdReadState& S = h->pcd_read;
  if (!J.parse_enqueued) return LSR_OK;
  LSR_HIP(hipStreamSynchronize(h->stream));
  int st;
  if (h->profile && (st = add_ms(S.ev[PcdReadState::EV_P0], S.ev[PcdReadState::EV_P1], &J.ms))) return st;
  const PcdReadStatus R = S.h_status.p[0];
  if (R.first_error != PCDR_NO_ERROR) {
    const unsigned long long at = file_offset + (R.first_error >> 3);
    const unsigned int kind = (unsigned int)(R.first_error & 7u);
    const char* why = kind == PCDR_ERR_TOO_LONG ? "a line longer than LSR_PCD_READ_MAX_LINE_BYTES"
                                                : (kind == PCDR_ERR_SHORT ? "a line with fewer values than the header's fields demand" : "a value that is not a number");
    set_last_error(std::string("PCD body: ") + why + ", line at byte offset " + std::to_string(at));
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (R.unresolved != J.unresolved_seen) {
    J.unresolved_seen = R.unresolved;
    J.h_flags.resize(J.keep);
    J.h_starts.resize(J.keep);
    J.h_records.resize(J.keep * J.step);
    LSR_HIP(hipMemcpyAsync(J.h_flags.data(), S.flags.p + J.done, J.keep, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipMemcpyAsync(J.h_starts.data(), S.line_start.p, J.keep * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipMemcpyAsync(J.h_records.data(), S.records.p + J.done * J.step, J.keep * J.step, hipMemcpyDeviceToHost, h->stream));
    if (!host_text) {
      J.h_text.resize(J.text_bytes);
      LSR_HIP(hipMemcpyAsync(J.h_text.data(), J.d_text, J.text_bytes, hipMemcpyDeviceToHost, h->stream));
      host_text = J.h_text.data();
    }
    LSR_HIP(hipStreamSynchronize(h->stream));
    std::string tok;
    for (size_t r = 0; r < J.keep; r++) {
      const unsigned int m = J.h_flags[r];
      if (!m) continue;
      for (int k = 0; k < 4; k++) {
        if (!(m & (1u << k)) || J.ap.out.off[k] < 0) continue;
        if (!host_token(host_text, J.text_bytes, J.h_starts[r], J.ap.tok[k], &tok)) { set_last_error("PCD body: an unresolved value was not found again"); return LSR_ERR_HIP; }
        const float v = std::strtof(tok.c_str(), nullptr);   // the grammar was checked on the device: a plain decimal number
        std::memcpy(J.h_records.data() + r * J.step + (size_t)J.ap.out.off[k], &v, 4);
      }
    }
    LSR_HIP(hipMemcpyAsync(S.records.p + J.done * J.step, J.h_records.data(), J.keep * J.step, hipMemcpyHostToDevice, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));
  }
  J.done += J.keep;
  J.keep = 0;
  J.parse_enqueued = false;
  return LSR_OK;
}

int too_few_lines(const PcdReadJob& J, unsigned long long end_offset) {
  set_last_error("PCD body: " + std::to_string(J.done) + " point lines where POINTS says " + std::to_string(J.n_points) +
                 " (the text ends at byte offset " + std::to_string(end_offset) + ")");
  return LSR_ERR_INVALID_ARGUMENT;
}

int job_end(PcdReadJob& J, void* out_records, int out_on_device, size_t* n_out) {
  lsr_handle h = J.h;
  PcdReadState& S = h->pcd_read;
  LSR_HIP(hipMemcpyAsync(out_records, S.records.p, J.n_points * J.step, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  S.parse_ms = J.ms;
  S.inflate_ms = J.inflate_ms;
  S.unresolved = (int)std::min<unsigned int>(J.unresolved_seen, (unsigned int)INT32_MAX);
  *n_out = J.n_points;
  return LSR_OK;
}

int check_read_args(const void* out_records, size_t capacity_points, const lsr_pc2_layout* out_layout, const size_t* n_out) {
  if (!n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!out_records) return LSR_OK;
  int st = check_out_layout(out_layout);
  if (st) return st;
  (void)capacity_points;   // a bound, not a count: the count is the file's, and load / decode hold it against the bound
  return arg_error(check_records(out_records, 0, MAP_RECORD_LIMIT, true, "out_records"));
}

// DATA binary_compressed: the two size words at the head of the body (words: its first 8 bytes, read only when the body has them)
// held against the header and against the body_bytes that lie behind the DATA line
int compressed_sizes(const PcdHeader& H, const unsigned char* words, unsigned long long body_bytes, size_t* n_stream, size_t* n_out) {
  if (body_bytes < 8) { set_last_error("PCD body: shorter than the two size words of DATA binary_compressed"); return LSR_ERR_INVALID_ARGUMENT; }
  uint64_t c = 0, u = 0;
  for (int i = 0; i < 4; i++) { c |= (uint64_t)words[i] << (8 * i); u |= (uint64_t)words[4 + i] << (8 * i); }
  if (c > (uint64_t)INT32_MAX || u > (uint64_t)INT32_MAX) {
    set_last_error("PCD body: compressed_size or uncompressed_size above 2^31 - 1");
    return LSR_ERR_INDEX_OVERFLOW;
  }
  const uint64_t image = H.info.n_points * (uint64_t)H.info.point_step;
  if (u != image) {
    set_last_error("PCD body: uncompressed_size " + std::to_string(u) + " where POINTS x record bytes is " + std::to_string(image));
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (c == 0) { set_last_error("PCD body: compressed_size is 0"); return LSR_ERR_INVALID_ARGUMENT; }
  if (c > body_bytes - 8) {
    set_last_error("PCD body: compressed_size " + std::to_string(c) + " where " + std::to_string(body_bytes - 8) + " bytes follow the size words");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  *n_stream = (size_t)c;
  *n_out = (size_t)u;
  return LSR_OK;
}

int too_small() {
  set_last_error("output buffer too small");
  return LSR_ERR_INVALID_ARGUMENT;
}

// lsr_load_pcd; to_target: the records go to the object's own {32; 0,4,8,16} buffer (out_records and capacity are ignored)
int load_pcd(lsr_handle h, const char* path, void* out_records, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device,
             size_t* n_out, bool to_target) {
  PcdReadState& S = h->pcd_read;
  PcdInFile file;
  errno = 0;
  file.f = std::fopen(path, "rb");
  if (!file.f) return pcdr_io_error("cannot open", path);
  PcdReadJob J;
  int st;
  {
    // the head of the file until the header is whole: 4 KiB, then more (a header with thousands of fields), 1 MiB at the most
    std::vector<unsigned char> head;
    size_t want = 4096;
    for (;;) {
      const size_t have = head.size();
      head.resize(want);
      errno = 0;
      const size_t got = std::fread(head.data() + have, 1, want - have, file.f);
      if (got < want - have && std::ferror(file.f)) return pcdr_io_error("cannot read", path);
      head.resize(have + got);
      bool incomplete = false;
      st = pcd_parse_header(head.data(), head.size(), &J.H, &incomplete, S.read_compressed != 0);
      if (!incomplete || got < want - have || want >= ((size_t)1 << 20)) break;
      want *= 4;
    }
    if (st) return st;
  }
  const size_t n = (size_t)J.H.info.n_points;
  if (!out_records && !to_target) { *n_out = n; return LSR_OK; }
  if (to_target) {
    if ((st = S.target.reserve(n * 32))) return st;
    out_records = S.target.p;
    capacity_points = n;
    out_on_device = 1;
  }
  const bool compressed = J.H.info.data_kind == 2;
  size_t n_stream = 0, n_image = 0;
  if (compressed) {
    // the size words are held against the file's length before anything else of the body is read
    errno = 0;
    if (fseeko(file.f, 0, SEEK_END) != 0) return pcdr_io_error("cannot seek in", path);
    const off_t end = ftello(file.f);
    if (end < 0) return pcdr_io_error("cannot seek in", path);
    const unsigned long long body_bytes = (unsigned long long)end > J.H.info.data_offset ? (unsigned long long)end - J.H.info.data_offset : 0;
    if (fseeko(file.f, (off_t)J.H.info.data_offset, SEEK_SET) != 0) return pcdr_io_error("cannot seek in", path);
    unsigned char words[8] = {0};
    if (body_bytes >= 8 && std::fread(words, 1, 8, file.f) != 8) return pcdr_io_error("cannot read", path);
    if ((st = compressed_sizes(J.H, words, body_bytes, &n_stream, &n_image))) return st;
  }
  if (capacity_points < n) return too_small();
  if (!compressed && fseeko(file.f, (off_t)J.H.info.data_offset, SEEK_SET) != 0) return pcdr_io_error("cannot seek in", path);
  if ((st = job_begin(J, h, out_layout))) return st;
  StreamDrain drain{h->stream};   // (destroyed before `file` and before J's host buffers: nothing is in flight when they go)
  const size_t P = (size_t)S.piece_bytes;
  unsigned long long file_off = J.H.info.data_offset;   // of the first byte of the buffer in hand

  if (compressed) {
    // the whole stream into HBM, piece k + 1 read while piece k is copied; then one inflate
    const size_t piece = std::min(P, n_stream);
    for (int par = 0; par < 2; par++)
      if ((st = S.pin[par].reserve(piece))) return st;
    if ((st = S.text.reserve(n_stream))) return st;
    auto read_piece = [&](int par, size_t first) -> int {
      const size_t cnt = std::min(piece, n_stream - first);
      errno = 0;
      if (std::fread(S.pin[par].p, 1, cnt, file.f) != cnt) return pcdr_io_error("cannot read", path);
      return LSR_OK;
    };
    if ((st = read_piece(0, 0))) return st;
    int par = 0;
    for (size_t sent = 0; sent < n_stream; par ^= 1) {
      const size_t cnt = std::min(piece, n_stream - sent);
      LSR_HIP(hipMemcpyAsync(S.text.p + sent, S.pin[par].p, cnt, hipMemcpyHostToDevice, h->stream));
      if (sent + cnt < n_stream && (st = read_piece(par ^ 1, sent + cnt))) return st;
      LSR_HIP(hipStreamSynchronize(h->stream));
      sent += cnt;
    }
    if ((st = pcd_lzf_inflate(S, S.text.p, n_stream, n_image, n, J.bp, S.records.p, file_off + 8, h->profile ? &J.inflate_ms : nullptr, h->stream)))
      return st;
    J.done = n;
    return job_end(J, out_records, out_on_device, n_out);
  }

  if (J.H.info.data_kind == 1) {
    const size_t rb = J.bp.rec_bytes, per_piece = std::max<size_t>(1, P / rb);
    for (int par = 0; par < 2; par++)
      if ((st = S.pin[par].reserve(per_piece * rb))) return st;
    if ((st = S.text.reserve(per_piece * rb))) return st;
    auto read_piece = [&](int par, size_t first) -> int {
      const size_t cnt = std::min(per_piece, n - first);
      errno = 0;
      if (std::fread(S.pin[par].p, 1, cnt * rb, file.f) != cnt * rb) {
        if (std::ferror(file.f)) return pcdr_io_error("cannot read", path);
        set_last_error("PCD body: shorter than POINTS records");
        return LSR_ERR_INVALID_ARGUMENT;
      }
      return LSR_OK;
    };
    if ((st = read_piece(0, 0))) return st;
    int par = 0;
    while (J.done < n) {
      const size_t cnt = std::min(per_piece, n - J.done);
      LSR_HIP(hipMemcpyAsync(S.text.p, S.pin[par].p, cnt * rb, hipMemcpyHostToDevice, h->stream));
      if ((st = pcd_read_binary(S.text.p, cnt, J.bp, S.records.p + J.done * J.step, h->stream))) return st;
      if (J.done + cnt < n && (st = read_piece(par ^ 1, J.done + cnt))) return st;
      LSR_HIP(hipStreamSynchronize(h->stream));
      J.done += cnt;
      par ^= 1;
    }
    return job_end(J, out_records, out_on_device, n_out);
  }

  // ASCII: a piece is the bytes up to the last newline of a buffer; what lies behind it is carried, without its leading blanks, to
  // the head of the next buffer (at most a line: PCDR_MAX_LINE bytes)
  for (int par = 0; par < 2; par++)
    if ((st = S.pin[par].reserve(P + PCDR_MAX_LINE))) return st;
  if ((st = S.text.reserve(P + PCDR_MAX_LINE))) return st;
  size_t carry = 0, got = 0;
  bool eof = false;
  auto read_into = [&](int par, size_t at) -> int {
    errno = 0;
    got = std::fread(S.pin[par].p + at, 1, P, file.f);
    if (got < P) {
      if (std::ferror(file.f)) return pcdr_io_error("cannot read", path);
      eof = true;
    }
    return LSR_OK;
  };
  if ((st = read_into(0, 0))) return st;
  int par = 0;
  for (;;) {
    unsigned char* buf = S.pin[par].p;
    const size_t len = carry + got;
    size_t cut = len;
    if (!eof) {
      cut = 0;
      for (size_t i = len; i > 0; i--)
        if (buf[i - 1] == '\n') { cut = i; break; }
    }
    size_t tail = cut;
    while (tail < len && pcd_is_blank(buf[tail])) tail++;
    const size_t tail_len = len - tail;
    const bool tail_too_long = tail_len > (size_t)PCDR_MAX_LINE;   // no newline within a line's length of its first byte
    const bool was_eof = eof;
    if (!tail_too_long && tail_len) std::memcpy(S.pin[par ^ 1].p, buf + tail, tail_len);
    if (cut) LSR_HIP(hipMemcpyAsync(S.text.p, buf, cut, hipMemcpyHostToDevice, h->stream));
    if ((st = ascii_piece_launch(J, S.text.p, cut))) return st;
    // the next piece is read while this one is parsed, unless this one fills the cloud
    const bool more = !was_eof && !tail_too_long && J.done + J.keep < n;
    if (more && (st = read_into(par ^ 1, tail_len))) return st;
    if ((st = ascii_piece_finish(J, buf, file_off))) return st;
    if (J.done >= n) break;
    if (tail_too_long) {
      set_last_error("PCD body: a line longer than LSR_PCD_READ_MAX_LINE_BYTES, line at byte offset " + std::to_string(file_off + tail));
      return LSR_ERR_INVALID_ARGUMENT;
    }
    if (was_eof) return too_few_lines(J, file_off + len);
    file_off += tail;
    carry = tail_len;
    par ^= 1;
  }
  return job_end(J, out_records, out_on_device, n_out);
}

}  // namespace

extern "C" {

int lsr_parse_pcd_header(const void* bytes, size_t n_bytes, lsr_pcd_info* info) {
  if (!bytes || !info) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  PcdHeader H{};
  const int st = pcd_parse_header(bytes, n_bytes, &H);
  if (st == LSR_OK || (st == LSR_ERR_NOT_IMPLEMENTED && H.info.data_kind == 2)) *info = H.info;
  return st;
}

int lsr_decode_pcd(lsr_handle h, const void* image, size_t n_bytes, int on_device, void* out_records, size_t capacity_points,
                   const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!image) { set_last_error("null image"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_read_args(out_records, capacity_points, out_layout, n_out);
  if (st) return st;
  PcdReadState& S = h->pcd_read;
  PcdReadJob J;
  std::vector<unsigned char> head;
  const unsigned char* host_image = on_device ? nullptr : static_cast<const unsigned char*>(image);
  if (on_device) {
    // the head of the image, for the header: 4 KiB, then 1 MiB
    for (size_t want : {(size_t)4096, (size_t)1 << 20}) {
      head.resize(std::min(want, n_bytes));
      LSR_HIP(hipMemcpyAsync(head.data(), image, head.size(), hipMemcpyDeviceToHost, h->stream));
      LSR_HIP(hipStreamSynchronize(h->stream));
      bool incomplete = false;
      st = pcd_parse_header(head.data(), head.size(), &J.H, &incomplete, S.read_compressed != 0);
      if (!incomplete || head.size() == n_bytes) break;
    }
  } else {
    st = pcd_parse_header(image, n_bytes, &J.H, nullptr, S.read_compressed != 0);
  }
  if (st) return st;
  const size_t n = (size_t)J.H.info.n_points, body_off = (size_t)J.H.info.data_offset, body = n_bytes - body_off;
  if (body >= ((size_t)1 << 32)) { set_last_error("a body of 2^32 bytes or more: read the file with lsr_load_pcd"); return LSR_ERR_INDEX_OVERFLOW; }
  if (!out_records) { *n_out = n; return LSR_OK; }
  const bool compressed = J.H.info.data_kind == 2;
  size_t n_stream = 0, n_image = 0;
  if (compressed) {
    unsigned char words[8] = {0};
    if (body >= 8) {
      if (on_device) {
        LSR_HIP(hipMemcpyAsync(words, static_cast<const unsigned char*>(image) + body_off, 8, hipMemcpyDeviceToHost, h->stream));
        LSR_HIP(hipStreamSynchronize(h->stream));
      } else {
        std::memcpy(words, host_image + body_off, 8);
      }
    }
    if ((st = compressed_sizes(J.H, words, body, &n_stream, &n_image))) return st;
  }
  if (capacity_points < n) return too_small();
  if (J.H.info.data_kind == 1 && body < n * (size_t)J.H.info.point_step) { set_last_error("PCD body: shorter than POINTS records"); return LSR_ERR_INVALID_ARGUMENT; }
  if (J.H.info.data_kind == 0 && body == 0) { J.n_points = n; return too_few_lines(J, n_bytes); }
  if ((st = job_begin(J, h, out_layout))) return st;
  StreamDrain drain{h->stream};
  const unsigned char* d_body = static_cast<const unsigned char*>(image) + body_off;
  const size_t used = compressed ? 8 + n_stream : (J.H.info.data_kind == 1 ? n * (size_t)J.H.info.point_step : body);
  if (!on_device) {
    if ((st = S.text.reserve(used))) return st;
    LSR_HIP(hipMemcpyAsync(S.text.p, host_image + body_off, used, hipMemcpyHostToDevice, h->stream));
    d_body = S.text.p;
  }
  if (compressed) {
    if ((st = pcd_lzf_inflate(S, d_body + 8, n_stream, n_image, n, J.bp, S.records.p, body_off + 8, h->profile ? &J.inflate_ms : nullptr, h->stream)))
      return st;
    J.done = n;
  } else if (J.H.info.data_kind == 1) {
    if ((st = pcd_read_binary(d_body, n, J.bp, S.records.p, h->stream))) return st;
    J.done = n;
  } else {
    if ((st = ascii_piece_launch(J, d_body, body))) return st;
    if ((st = ascii_piece_finish(J, host_image ? host_image + body_off : nullptr, body_off))) return st;
    if (J.done < n) return too_few_lines(J, n_bytes);
  }
  return job_end(J, out_records, out_on_device, n_out);
}

int lsr_load_pcd(lsr_handle h, const char* path, void* out_records, size_t capacity_points, const lsr_pc2_layout* out_layout,
                 int out_on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!path) { set_last_error("null path"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_read_args(out_records, capacity_points, out_layout, n_out);
  if (st) return st;
  return load_pcd(h, path, out_records, capacity_points, out_layout, out_on_device, n_out, false);
}

int lsr_set_input_target_pcd(lsr_handle h, const char* path, size_t* n_points) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_points) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  static const lsr_pc2_layout xyzi = {32, 0, 4, 8, 16};   // pcl::PointXYZI, what the map was saved from
  size_t n = 0;
  int st = load_pcd(h, path, nullptr, 0, &xyzi, 1, &n, true);
  if (st) return st;
  if ((st = lsr_set_input_target_device(h, h->pcd_read.target.p, 32, n))) return st;
  *n_points = n;
  return LSR_OK;
}

}  // extern "C"
