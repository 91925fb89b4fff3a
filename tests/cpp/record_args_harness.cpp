// TEST INFRASTRUCTURE: csrc/record_args.hpp as a program of its own, for tests/test_record_args_cpu.py.  The header promises to need no
// HIP: this file is compiled by plain g++ -Wall -Werror (and once more with -fsanitize=address,undefined).  It evaluates one check per
// line of standard input and prints one line of statuses per check; the expected statuses live in tests/record_args_cases.py.
// Pointers are given as integers and are never dereferenced.
//   layout  step ox oy oz oi          -> "<xyz> <full> <out>"     check_layout_xyz, check_layout_arg, check_out_layout_arg
//   stride  s                         -> "<status>"               check_stride_arg
//   records ptr n limit align4        -> "<status>"               check_records; limit: ingest | map
//   inout   in out n step             -> "<status>"               check_records_in_out
//   overlap a a_bytes b b_bytes       -> "0" | "1"                ranges_overlap
//   frames  stride lists n {ptr cnt}  -> "<status>"               check_frame_list; lists: 1 = the three arrays are there, 0 = they are null
// A status that is not LSR_OK must come with both texts; "bad" is printed instead of it otherwise.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../lidarslam_ros2_amd/csrc/record_args.hpp"

namespace {

const void* as_ptr(unsigned long long v) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(v)); }

std::string show(const lsr::ArgStatus& a) {
  const bool failed = static_cast<bool>(a);
  if (failed != (a.status != LSR_OK)) return "bad";
  if (failed && (!a.what || !a.why || !a.what[0] || !a.why[0])) return "bad";
  return std::to_string(a.status);
}

}  // namespace

int main() {
  std::string line;
  int n_lines = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    n_lines++;
    if (kind == "layout") {
      long long step, ox, oy, oz, oi;
      in >> step >> ox >> oy >> oz >> oi;
      const lsr_pc2_layout L{(uint32_t)step, (uint32_t)ox, (uint32_t)oy, (uint32_t)oz, (int32_t)oi};
      std::cout << show(lsr::check_layout_xyz(&L)) << " " << show(lsr::check_layout_arg(&L)) << " " << show(lsr::check_out_layout_arg(&L)) << "\n";
    } else if (kind == "nolayout") {
      std::cout << show(lsr::check_layout_xyz(nullptr)) << " " << show(lsr::check_layout_arg(nullptr)) << " "
                << show(lsr::check_out_layout_arg(nullptr)) << "\n";
    } else if (kind == "stride") {
      unsigned long long s;
      in >> s;
      std::cout << show(lsr::check_stride_arg((size_t)s)) << "\n";
    } else if (kind == "records") {
      unsigned long long p, n;
      std::string limit;
      int align4;
      in >> p >> n >> limit >> align4;
      const lsr::RecordLimit& lim = limit == "map" ? lsr::MAP_RECORD_LIMIT : lsr::INGEST_RECORD_LIMIT;
      std::cout << show(lsr::check_records(as_ptr(p), (size_t)n, lim, align4 != 0, "records")) << "\n";
    } else if (kind == "inout") {
      unsigned long long a, b, n, step;
      in >> a >> b >> n >> step;
      std::cout << show(lsr::check_records_in_out(as_ptr(a), as_ptr(b), (size_t)n, (size_t)step)) << "\n";
    } else if (kind == "overlap") {
      unsigned long long a, an, b, bn;
      in >> a >> an >> b >> bn;
      std::cout << (lsr::ranges_overlap(as_ptr(a), (size_t)an, as_ptr(b), (size_t)bn) ? 1 : 0) << "\n";
    } else if (kind == "frames") {
      unsigned long long stride;
      int lists, n;
      in >> stride >> lists >> n;
      std::vector<const void*> frames;
      std::vector<size_t> counts;
      unsigned long long p, c;
      while (in >> p >> c) { frames.push_back(as_ptr(p)); counts.push_back((size_t)c); }
      frames.push_back(nullptr);   // (never empty: data() below is a pointer)
      counts.push_back(0);
      const float poses[16] = {0};
      size_t total = 0, biggest = 0;
      const lsr::ArgStatus a = lists ? lsr::check_frame_list(n, frames.data(), counts.data(), (size_t)stride, poses, &total, &biggest)
                                     : lsr::check_frame_list(n, nullptr, nullptr, (size_t)stride, nullptr, &total, &biggest);
      std::cout << show(a);
      if (!a) std::cout << " " << total << " " << biggest;
      std::cout << "\n";
    } else {
      std::fprintf(stderr, "record_args_harness: unknown check '%s'\n", kind.c_str());
      return 2;
    }
  }
  std::fprintf(stderr, "record_args_harness: %d checks\n", n_lines);
  return 0;
}
