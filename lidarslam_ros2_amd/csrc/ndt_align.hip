// The host driver of NDT (the kernels: ndt.hip): launch geometry, the table mode of a pass, the launch-chain streams of a batch lead,
// the launch feeder and align for a set of registrations — and the NDT inspection entries of the C ABI, which drive the same pieces.
// Host-side orchestration only; the two kernels here are the one-thread probes that measure how streams map to hardware queues.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <limits>
#include <thread>

#include "api_internal.hpp"

using namespace lsr;

namespace {

// Workgroups per registration.  A single registration spreads one point per thread over as many CUs as
// it can (latency); a batch wants ~4 resident workgroups per CU in total and lets every thread stride
// over several points, which amortises the reduction and the partial-row traffic (throughput).
// Compute units of the device (256 on MI355X).
int device_cus(int device) {
  static int cached[64] = {};
  if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
  if (device >= 0 && device < 64) cached[device] = v;
  return v;
}

// Workgroups per registration.  Every workgroup of a pass pays the fixed head of the launch (totals of the previous pass,
// controller step, next request: 2.5-4 us) before it evaluates a point, so a pass never launches more workgroups than the
// chip holds at once — two 512-thread workgroups of the quad kernel (128 points each) or of the lane kernel per CU, one of its
// 1024-thread workgroups — and lets each of them walk several batches of points instead.
// `threads`: THREADS per workgroup; `points`: source points a workgroup takes per trip (quad kernel: threads / 4).
constexpr int NDT_LANE_SINGLE_MIN = 65536;   // source points from which a single registration uses the lane kernel
int ndt_resident_wgs(int device, int threads) {
  // two 512-thread workgroups per CU (128 VGPRs per lane: four waves per SIMD; the lane kernel's LDS table + staging tiles fit twice),
  // one of 1024 threads.  (Until round 5 this returned 2048 / threads = 4 for 512: more workgroups than are ever co-resident, each of
  // them paying the head.  Measured on the 64-candidate chain: 1.46 ms with 4, 1.46 ms with 2, 2.04 ms with 1.)
  // Below 512 threads (the quad kernel with 64 points per workgroup: 256 threads, LSR_NDT_WORKGROUP=64) occupancy decides again:
  // 2048 / threads workgroups fill the same four waves per SIMD (the measurement above covers 512 and 1024 only).
  const int by_size = threads >= 1024 ? 1 : threads >= 512 ? 2 : 2048 / std::max(64, threads);
  return device_cus(device) * by_size;
}
int ndt_nblocks(size_t n, int device, int batch, int threads, int points) {
  int nb = (int)((n + points - 1) / points);
  const int share = std::max(1, ndt_resident_wgs(device, threads) / std::max(1, batch));
  nb = std::max(1, std::min(nb, std::min(share, NDT_MAX_BLOCKS)));
  return nb;
}
// workgroup geometry of a launch configuration
int cfg_wg_threads(const NdtLaunchCfg& cfg) { return cfg.quad ? 4 * cfg.threads : cfg.threads; }
int cfg_wg_points(const NdtLaunchCfg& cfg) { return (!cfg.quad && cfg.split) ? cfg.threads / 2 : cfg.threads; }

// LDS a workgroup may use on this device (hipDeviceAttributeMaxSharedMemoryPerBlock; 160 KiB on gfx950): the table modes that
// stage into LDS are only chosen when their buffers fit, anything else reads the global table.
int device_lds_bytes(int device) {
  static int cached[64] = {};
  if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
  // one workgroup may use a CU's whole LDS on AMD hardware: the larger of the two attributes (runtimes differ in which one
  // reports the 160 KiB of gfx950); 64 KiB when neither answers
  int per_block = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) per_block = 0;
  if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) != hipSuccess) per_cu = 0;
  int v = std::max(per_block, per_cu);
  if (v <= 0) v = 64 * 1024;
  if (device >= 0 && device < 64) cached[device] = v;
  return v;
}
constexpr int NDT_QUAD_STATIC_LDS = 32 * 1024;   // static LDS of the quad kernel next to its table (27 KiB + margin)
constexpr int NDT_LANE_STATIC_LDS = 6 * 1024;    // ... of the lane kernel (bins, state image; its staging tiles are dynamic LDS)

void fill_problem(NdtProblem& P, lsr_handle h, NdtState* d_state, long long* d_bins, const NdtLaunchCfg& cfg) {
  const VoxelGridDev& g = h->target->grid;
  P.sx = h->source.x(); P.sy = h->source.y(); P.sz = h->source.z();
  P.n = (int)h->source.n;
  P.nblocks = ndt_nblocks(h->source.n, h->device, cfg.batch, cfg_wg_threads(cfg), cfg_wg_points(cfg));
  P.lds_image = g.lds_image.p;
  P.lds_map_bytes = g.lds_map_bytes;
  P.lds_bytes = g.lds_bytes;
  P.cell_slot = g.cell_slot.p;
  P.rec = g.rec.p;
  for (int k = 0; k < 3; k++) { P.min_b[k] = g.min_b[k]; P.max_b[k] = g.max_b[k]; }
  P.mul1 = g.div_b[0];
  P.mul2 = g.div_b[0] * g.div_b[1];
  P.leaf = g.leaf;
  P.st = d_state;
  P.bins = d_bins;
  P.mailbox = nullptr;
  // KDTREE: the 27-cell kernels with the kd-tree's radius test (ensure_ndt_grid built the centroids); resolution_ is a float member
  const bool kd = h->ndt.neighborhood == LSR_KDTREE && h->target->has_centroids;
  P.centroid = kd ? g.centroid.p : nullptr;
  P.radius2 = kd ? (float)((double)(float)h->ndt.resolution * (double)(float)h->ndt.resolution) : 0.f;
}

// Where the derivative pass reads the leaf records, and with which kernel.  grids: the batch's targets.
//  every table fits LDS            -> NDT_TAB_LDS   (quad kernel for one registration, one-lane kernel for a batch)
//  dense tables that do not fit    -> NDT_TAB_DENSE (global gathers; L2 resident at the reference's resolutions)
//  tables beyond 4 Mi cells        -> NDT_TAB_COMPACT (global gathers through cell_slot)
// table_mode: the lead object's LSR_NDT_TABLE_MODE override (-1 automatic).
void choose_table_mode(lsr_handle lead, lsr_handle* hs, int B, NdtLaunchCfg& cfg) {
  bool all_lds = true, all_dense = true;
  int lds_max = 0;
  for (int b = 0; b < B; b++) {
    const VoxelGridDev& g = hs[b]->target->grid;
    all_lds = all_lds && g.lds_bytes > 0;
    all_dense = all_dense && g.dense;
    lds_max = std::max(lds_max, g.lds_bytes);
  }
  const int lds_cap = device_lds_bytes(lead->device);
  const int override_mode = lead->ndt_table_mode;
  // four lanes per point for ONE registration (latency: a 30k-point scan on every CU); the lane kernel for candidate sets and
  // on request (LSR_NDT_QUAD = 0) — both return the same bits, so the choice is a matter of speed only.  Measured on cfg-4 sets of
  // 8 / 16 / 64 candidates (align stage, round 3's kernels): one lane per point 0.61 / 0.90 / 2.73 ms, four lanes 0.76 / 1.09 / 4.06 ms
  // ... and a single scan large enough to fill the chip with one lane per point takes the lane kernel too: cfg 5 (120k points,
  // dense global table) 9.4 us per pass with 512-thread workgroups against 16.1 us through the quad kernel (round 4)
  size_t n_max = 0;
  for (int b = 0; b < B; b++) n_max = std::max(n_max, hs[b]->source.n);
  const bool want_quad_single = (B == 1 && (lead->ndt_quad == 1 || (lead->ndt_quad < 0 && n_max < (size_t)NDT_LANE_SINGLE_MIN)));
  // 512 threads per workgroup (1024 on request).  A workgroup's waves share ONE compute unit: 1024 threads are four waves per SIMD
  // whatever the size of the set, 512 are two and twice the workgroups — cfg-4 sets of 4 / 8 / 16 / 64 members, align stage:
  // 0.48 / 0.50 / 0.71 / 1.98 ms with 1024 threads, 0.40 / 0.48 / 0.65 / 1.74 ms with 512 (two chains from 6 members on).
  // (DIRECT26's 27 neighbours per point do not fit the 128 registers a 1024-thread workgroup leaves a lane anyway.)
  const int lane_threads = (lead->ndt_threads == 512 || lead->ndt_threads == 1024) ? lead->ndt_threads : NDT_LANE_THREADS;
  const int static_lds = want_quad_single ? NDT_QUAD_STATIC_LDS : NDT_LANE_STATIC_LDS + ndt_lane_tile_bytes(lane_threads);
  const int table_cap = std::min(want_quad_single ? NDT_LDS_TABLE_MAX_QUAD : NDT_LDS_TABLE_MAX, lds_cap - static_lds);
  const bool lds_ok = all_lds && lds_max <= table_cap;
  int tab;
  if (override_mode == NDT_TAB_COMPACT) tab = NDT_TAB_COMPACT;
  else if (override_mode == NDT_TAB_DENSE && all_dense) tab = NDT_TAB_DENSE;
  else if (override_mode == NDT_TAB_LDS && lds_ok) tab = NDT_TAB_LDS;
  else if (lds_ok) tab = NDT_TAB_LDS;
  else tab = all_dense ? NDT_TAB_DENSE : NDT_TAB_COMPACT;   // measured: the pass is not gather bound
  cfg.tab = tab;
  if (std::getenv("LSR_DEBUG_TABLE")) {
    static int shown = 0;
    if (shown++ < 4) fprintf(stderr, "[lidarslam_reg] table mode %d for %d member(s): LDS image up to %d bytes (cap %d, static %d)\n", tab, B, lds_max, table_cap, static_lds);
  }
  cfg.quad = want_quad_single ? 1 : 0;
  cfg.lds_bytes = (tab == NDT_TAB_LDS) ? lds_max : 0;
  if (cfg.quad) cfg.threads = (lead->ndt_threads == 64 || lead->ndt_threads == 128) ? lead->ndt_threads : NDT_QUAD_POINTS;  // POINTS per workgroup
  else cfg.threads = lane_threads;
  // two waves per chunk (ndt.hip: SPLIT) for a single scan whose points, one lane each, leave the chip half empty but whose chunk
  // pairs still fit it at once: 65 536 .. resident workgroups x 256 points (cfg 5: 120 000 points = 469 workgroups of 512 threads).
  // LSR_NDT_SPLIT = 0 / 1 (key or environment preset) forces it off / on (on: any single registration that takes the 512-thread lane
  // kernel with a DIRECT neighbourhood: the KDTREE kernels have no split form).
  cfg.split = 0;
  if (!cfg.quad && B == 1 && cfg.threads == 512 && lead->ndt.neighborhood != LSR_KDTREE) {
    // measured (cfg 5, 120 000 points, res 2.0 / 1.0): 9.25 / 9.33 us per pass split against 9.14 / 9.08 us with one wave per chunk —
    // the pass is bound by its fixed chain (boundary, head read, controller: ~5.5 us), not by the point loop the split halves; the
    // barrier and the second copy of the gathers eat what the shorter per-wave chain gives.  Automatic = off; kept as an A/B form
    // (same bits: tests/test_ndt_gpu.py) with its counters in profiles/r06_pmc_cfg5.md.
    cfg.split = lead->ndt_split >= 0 ? lead->ndt_split : 0;
  }
}

// The host feeds the launch chain and watches the mailboxes the chain writes into host memory (NdtMailbox, one per
// registration of the batch): workgroup 0 of every launch reports its sequence number, the launch in which a
// registration's controller finishes publishes its result and raises its `done`.  Launch `seq` consumes the rows of
// launch seq-1 (ndt.hip), so an align of E derivative passes takes E+1 launches.  The host keeps a couple of launches
// queued ahead of the device and never synchronises the stream or copies state back inside the chain; after the last
// `done` at most LOW_WATER + REFILL queued launches remain, which exit at their head.
// on_poll (nullable): called between polls while the chain runs (the eager fitness dispatch of a candidate set hangs off it).
// nb_full > 0 (lane kernel, candidate sets): the launches are widened as members finish — grid.x = resident workgroups /
// members still running, at most nb_full (= one trip per lane for the largest member); the canonical sum does not depend on it.
// --- launch-chain streams -------------------------------------------------------------------------------------------------
// Two HIP streams run concurrently only when the runtime has mapped them to different hardware queues; mapped to the same
// queue their launches serialise AND every switch between them costs a signal round trip (measured: 60 us per switch, a
// three-chain set took twice as long as one chain when two chains shared a queue).  The mapping cannot be queried, so it is
// MEASURED once per stream: a kernel on stream a spins (bounded) on a flag that a kernel enqueued AFTERWARDS on stream b sets.
__global__ void chain_probe_wait(unsigned int* flag, unsigned int* seen, unsigned long long budget) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
  unsigned int v = 0;
  while ((v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 &&
         __builtin_amdgcn_s_memrealtime() - t0 < budget) __builtin_amdgcn_s_sleep(8);
  *seen = v ? 1u : 2u;
}
__global__ void chain_probe_set(unsigned int* flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1: b's kernel ran while a's was running; 0: it did not within 200 us (same hardware queue); < 0: error (negated status)
int streams_run_concurrently(hipStream_t a, hipStream_t b, unsigned int* d_words /* 2 */) {
  // the flag is cleared and BOTH streams are idle before the two kernels go out (b's kernel may overtake anything a still holds)
  if (hipMemsetAsync(d_words, 0, 8, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -LSR_ERR_HIP;
  hipLaunchKernelGGL(chain_probe_wait, dim3(1), dim3(1), 0, a, d_words, d_words + 1, 20000ull);
  hipLaunchKernelGGL(chain_probe_set, dim3(1), dim3(1), 0, b, d_words);
  unsigned int seen = 0;
  if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess ||
      hipMemcpy(&seen, d_words + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) return -LSR_ERR_HIP;
  return seen == 1u ? 1 : 0;
}

// The auxiliary streams of a batch lead, looked for once per handle: the side stream (grid refinement and fitness searches of a
// candidate set, under the launch chain) and up to two more launch-chain streams, each VERIFIED to run concurrently with the
// lead's stream and with the ones found before it.  A stream that fails the check is kept alive until the search ends, so
// that the runtime maps the next one to another hardware queue.  When no concurrent side stream turns up an unverified one
// is used (correct, just not overlapped); chain streams are only ever verified ones.
int ensure_aux_streams(lsr_handle lead) {
  if (lead->chain_probed) return LSR_OK;
  lsr::DevBuf<unsigned int> words;
  int st;
  if ((st = words.reserve(2))) return st;
  std::vector<hipStream_t> rejected, found;
  // (Round 5 measured a lowest-priority side stream — hipStreamCreateWithPriority — for the grid refinement and the fitness searches:
  // the chain launches were disturbed just the same and the side work itself was starved: align + fitness of an 8-candidate share
  // 1.26-1.38 ms against 0.76-0.95 ms.  Not used.)
  for (int tries = 0; tries < 10 && (int)found.size() < 3; tries++) {
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
    bool ok = streams_run_concurrently(lead->stream, s, words.p) == 1;
    for (size_t c = 0; ok && c < found.size(); c++) ok = streams_run_concurrently(found[c], s, words.p) == 1;
    if (ok) found.push_back(s); else rejected.push_back(s);
  }
  for (hipStream_t s : rejected) (void)hipStreamDestroy(s);
  (void)hipStreamSynchronize(lead->stream);
  // from here on a failure must not leak what was found (and must not leave half of it on the handle: the next call probes again)
  auto give_up = [&](const char* what) {
    for (hipStream_t s : found) if (s) (void)hipStreamDestroy(s);
    if (found.empty() && lead->side_stream) (void)hipStreamDestroy(lead->side_stream);
    lead->side_stream = nullptr;
    for (int c = 0; c < 3; c++) {
      lead->chain_stream[c] = nullptr;
      if (lead->chain_ev[c]) { (void)hipEventDestroy(lead->chain_ev[c]); lead->chain_ev[c] = nullptr; }
    }
    lead->n_chain_streams = 0;
    set_last_error(std::string("auxiliary streams of a batch lead: ") + what);
    return LSR_ERR_HIP;
  };
  size_t k = 0;
  if (!found.empty()) lead->side_stream = found[k++];
  else if (hipStreamCreateWithFlags(&lead->side_stream, hipStreamNonBlocking) != hipSuccess) return give_up("no side stream");
  lead->n_chain_streams = 0;
  for (; k < found.size(); k++) {
    hipEvent_t ev = nullptr;
    if (lead->n_chain_streams < 3 && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      lead->chain_stream[lead->n_chain_streams] = found[k]; lead->chain_ev[lead->n_chain_streams] = ev; lead->n_chain_streams++;
    } else { (void)hipStreamDestroy(found[k]); found[k] = nullptr; }
  }
  if (!lead->side_ev && hipEventCreateWithFlags(&lead->side_ev, hipEventDisableTiming) != hipSuccess) return give_up("event");
  if (!lead->side_fork_ev && hipEventCreateWithFlags(&lead->side_fork_ev, hipEventDisableTiming) != hipSuccess) return give_up("event");
  if (!lead->chain_fork_ev && hipEventCreateWithFlags(&lead->chain_fork_ev, hipEventDisableTiming) != hipSuccess) return give_up("event");
  lead->chain_probed = true;
  if (std::getenv("LSR_DEBUG_STREAMS"))
    fprintf(stderr, "[lidarslam_reg] aux streams of handle %p: %zu verified concurrent, %zu rejected, %d chain stream(s)\n", (void*)lead,
            found.size(), rejected.size(), lead->n_chain_streams);
  return LSR_OK;
}

// how many independent launch chains a set of B registrations runs as (env LSR_NDT_CHAINS = 1..3 forces it for B >= 2*chains; at most two verified chain streams exist next to the lead's own)
int ndt_chain_count(int B) {
  static const int forced = [] { const char* e = std::getenv("LSR_NDT_CHAINS"); return e ? std::atoi(e) : 0; }();
  // measured (cfg-4 sets, align stage, 1 -> 2 chains, 512-thread workgroups): 4 members +13 %, 6 members 0 %, 8 / 12 / 16 members
  // -3 / -9 / -13 %; with 1024-thread workgroups 24 / 32 / 48 / 64 members -17 / -10 / -10 / -9 %
  int n = forced > 0 ? std::min(forced, 3) : (B >= 6 ? 2 : 1);
  while (n > 1 && B < 2 * n) n--;
  return n;
}

// n_chains > 1 (small candidate sets): the members are dealt to n_chains independent launch chains, chain c covering members
// [chain_first[c], chain_first[c+1]) on streams[c].  A launch of a small set is mostly fixed latency (the launch boundary and
// the head: bank fold + controller), which the other chain's launch hides; the answer of a member does not depend on which
// launches carry it (canonical sums), so the split changes no bit.
int run_ndt_feeder(lsr_handle h, const NdtProblem* d_probs, const NdtProblem* h_probs, const NdtLaunchCfg& cfg_in, int first, int hard_cap,
                   unsigned int token, int* launches_out, const std::function<int()>* on_poll = nullptr, int nb_full = 0,
                   int n_chains = 1, const int* chain_first = nullptr, const hipStream_t* streams = nullptr) {
  constexpr int MAX_CHAINS = 4;
  struct Chain { int b0, b1, n_done, launched; bool over; hipStream_t stream; NdtLaunchCfg cfg; };
  Chain ch[MAX_CHAINS];
  const int one_first[2] = {0, cfg_in.batch};
  if (n_chains <= 1 || !chain_first || !streams) { n_chains = 1; chain_first = one_first; streams = &h->stream; }
  if (n_chains > MAX_CHAINS) { set_last_error("too many launch chains"); return LSR_ERR_INVALID_ARGUMENT; }
  const int resident = ndt_resident_wgs(h->device, cfg_wg_threads(cfg_in));
  // spin: two launches queued ahead are enough; yield / sleep give the core away between polls, so more launches are
  // kept queued to ride out the scheduler's latency (surplus launches exit at their head, ~2 us each)
  const int wait_mode = h->scratch.wait_mode;
  const int LOW_WATER = (wait_mode == WAIT_SPIN) ? 2 : (wait_mode == WAIT_YIELD ? 4 : 16), REFILL = (wait_mode == WAIT_SLEEP) ? 8 : 2;
  const int batch = cfg_in.batch;
  const NdtMailbox* mb = h->mailbox.p;
  const NdtProblem* h_single = (batch == 1) ? h_probs : nullptr;  // a single registration travels in the kernel arguments
  int st;
  for (int c = 0; c < n_chains; c++) {
    Chain& C = ch[c];
    C.b0 = chain_first[c]; C.b1 = chain_first[c + 1]; C.n_done = C.b0; C.over = false; C.stream = streams[c];
    C.cfg = cfg_in; C.cfg.batch = C.b1 - C.b0;
    C.launched = std::max(1, std::min(first, hard_cap));
    if ((st = ndt_launch_evals(d_probs + C.b0, h_single, C.cfg, 0, C.launched, C.stream))) return st;
  }
  unsigned long long last_progress = 0;
  auto t_progress = std::chrono::steady_clock::now();
  int chains_left = n_chains;
  for (unsigned long long spins = 1; chains_left > 0; spins++) {
    unsigned long long pr_sum = 0;
    for (int c = 0; c < n_chains; c++) {
      Chain& C = ch[c];
      if (C.over) continue;
      while (C.n_done < C.b1 && __atomic_load_n(&mb[C.n_done].done, __ATOMIC_ACQUIRE) == token) C.n_done++;  // [b0, n_done) have raised their flag
      if (C.n_done == C.b1) { C.over = true; chains_left--; continue; }
      // every registration of a launch advances together: the first unfinished one tells how far the device is
      const unsigned long long pr = __atomic_load_n(&mb[C.n_done].progress, __ATOMIC_RELAXED);
      pr_sum += pr;
      const int entered = ((unsigned int)(pr >> 32) == token) ? (int)(unsigned int)pr : -1;  // -1: nothing of this align yet
      if (C.launched < hard_cap && C.launched - 1 - entered < LOW_WATER) {
        const int k = std::min(REFILL, hard_cap - C.launched);
        if (nb_full > 0 && batch > 1) {
          int running = 0;   // over all chains: they share the chip
          for (int b = 0; b < batch; b++) running += (__atomic_load_n(&mb[b].done, __ATOMIC_RELAXED) != token);
          C.cfg.max_blocks = std::max(cfg_in.max_blocks, std::min(nb_full, resident / std::max(1, running)));
        }
        if ((st = ndt_launch_evals(d_probs + C.b0, h_single, C.cfg, C.launched, k, C.stream))) return st;
        C.launched += k;
        continue;
      }
      if (C.launched >= hard_cap && entered >= hard_cap - 1) {  // the last permitted launch has started: let it finish
        LSR_HIP(hipStreamSynchronize(C.stream));
        while (C.n_done < C.b1 && __atomic_load_n(&mb[C.n_done].done, __ATOMIC_ACQUIRE) == token) C.n_done++;
        if (C.n_done == C.b1) { C.over = true; chains_left--; continue; }
        set_last_error("NDT controller did not finish within the launch cap");
        return LSR_ERR_HIP;
      }
    }
    if (chains_left == 0) break;
    if ((spins & 0x3FFF) == 0 || wait_mode == WAIT_SLEEP) {  // a device that stops making progress must not hang the caller forever
      const auto now = std::chrono::steady_clock::now();
      if (pr_sum != last_progress) { last_progress = pr_sum; t_progress = now; }
      if (std::chrono::duration<double>(now - t_progress).count() > 30.0) {
        const hipError_t e = hipStreamQuery(h->stream);
        set_last_error(std::string("NDT launch chain made no progress for 30 s (stream: ") + hipGetErrorString(e) + ")");
        return LSR_ERR_HIP;
      }
    }
    if (on_poll && (spins & 0xF) == 0 && (st = (*on_poll)())) return st;
    if (wait_mode == WAIT_YIELD) std::this_thread::yield();
    else if (wait_mode == WAIT_SLEEP) std::this_thread::sleep_for(std::chrono::microseconds(20));
    else __builtin_ia32_pause();
  }
  int launched = 0;
  for (int c = 0; c < n_chains; c++) launched = std::max(launched, ch[c].launched);
  *launches_out = launched;
  return LSR_OK;
}

int ndt_hard_cap(const NdtParamsHost& p) {
  // per Newton iteration: 1 first pass + <=10 trials + 1 Hessian recomputation; max_iter+2 iterations; + initial pass.
  // A search that runs to the tenth trial takes its Hessian from that trial's pass (PH_MT_LAST) and needs one launch less, so
  // this stays an upper bound; the searches that stop after 1-9 trials still reach 1 + 9 + 1.
  return (p.max_iterations + 2) * 12 + 5;
}

int ndt_min_evals(const NdtParamsHost& p) {
  // with a non-positive epsilon the loop can only stop on the iteration count: at least max_iter+2 line searches
  if (p.trans_eps <= 0) return p.max_iterations + 4;  // + the finalising launch
  return 8;
}

}  // namespace

// fitness_out (nullable): getFitnessScore(max_range) of every member as well (graph_based_slam_component.cpp:230-231 calls the two back
// to back).  For members whose neighbour grid is refined from their voxel grid the search of a member is enqueued on the side
// stream AS SOON AS ITS REGISTRATION HAS FINISHED, under the launch chain of the members still running; fitness_out[b] is NaN for
// a member that was not served that way (the caller falls back to lsr_get_fitness_score_batch for those).
int lsr::align_ndt_batch(lsr_handle* hs, int B, const float* guesses, float* finals, lsr_result* results, double* fitness_out,
                         double max_range) {
  lsr_handle lead = hs[0];
  if (fitness_out) for (int b = 0; b < B; b++) fitness_out[b] = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; b < B; b++) {
    lsr_handle h = hs[b];
    if (!h->target || h->target->n == 0) { set_last_error("align before setInputTarget"); return LSR_ERR_NO_TARGET; }
    if (!h->has_source) { set_last_error("align before setInputSource"); return LSR_ERR_NO_SOURCE; }
    if (h->ndt.neighborhood != lead->ndt.neighborhood) { set_last_error("batched handles must share the neighbourhood method"); return LSR_ERR_INVALID_ARGUMENT; }
    int st = ensure_ndt_grid(h);
    if (st) return st;
    if (h->target->grid.ncells == 0) {  // no finite target point: there is no table a lookup could read
      set_last_error("the input target holds no finite point");
      return LSR_ERR_NO_TARGET;
    }
  }
  // The shared launches run on the lead's stream; a member on another stream may still have its setInputSource /
  // setInputTarget kernels in flight there: order the lead's stream after each of them (event + stream wait, no host wait)
  int st;
  for (int b = 1; b < B; b++)
    if ((st = order_lead_after(lead->stream, hs[b]))) return st;
  if ((st = lead->d_state.reserve(2 * (size_t)B))) return st;
  if ((st = lead->d_prob.reserve(B))) return st;
  {  // pinned, mapped: a set's init launch reads the members' records straight out of these arrays (ndt_init_batch)
    const NdtState* hs0 = lead->h_state.p; const NdtProblem* hp0 = lead->h_prob.p;
    if ((st = lead->h_state.reserve(2 * (size_t)B, hipHostMallocMapped))) return st;
    if ((st = lead->h_prob.reserve(B, hipHostMallocMapped))) return st;
    if (lead->h_state.p != hs0 || !lead->h_state_dev) LSR_HIP(hipHostGetDevicePointer((void**)&lead->h_state_dev, lead->h_state.p, 0));
    if (lead->h_prob.p != hp0 || !lead->h_prob_dev) LSR_HIP(hipHostGetDevicePointer((void**)&lead->h_prob_dev, lead->h_prob.p, 0));
  }
  // larger sets run as several independent launch chains (run_ndt_feeder), each on a stream of its own that starts behind
  // everything the lead's stream holds at this point (the members' builds and uploads) and does its own state uploads
  int n_chains = ndt_chain_count(B);
  if (B > 1 && (st = ensure_aux_streams(lead))) return st;   // once per lead handle
  n_chains = std::min(n_chains, 1 + lead->n_chain_streams);
  int chain_first[5] = {0, B, B, B, B};
  hipStream_t chain_streams[4] = {lead->stream, nullptr, nullptr, nullptr};
  // Every way out of this function after the fork joins the chain streams back into the lead's stream: whatever follows there (the
  // next align's state upload, a release of the banks) stays behind launches, sorts and uploads still queued on a chain stream.
  struct ChainJoin {
    lsr_handle lead; int n = 1; bool joined = false;
    bool join() {   // false: a stream had to be drained by the host instead
      if (joined) return true;
      joined = true;
      bool ok = true;
      for (int c = 1; c < n; c++)
        if (hipEventRecord(lead->chain_ev[c - 1], lead->chain_stream[c - 1]) != hipSuccess ||
            hipStreamWaitEvent(lead->stream, lead->chain_ev[c - 1], 0) != hipSuccess) {
          (void)hipStreamSynchronize(lead->chain_stream[c - 1]);
          ok = false;
        }
      return ok;
    }
    ~ChainJoin() { (void)join(); }
  } chain_join{lead};
  if (n_chains > 1) {
    LSR_HIP(hipEventRecord(lead->chain_fork_ev, lead->stream));
    for (int c = 0; c <= n_chains; c++) chain_first[c] = (int)((long)B * c / n_chains);
    chain_join.n = n_chains;
    for (int c = 1; c < n_chains; c++) {
      chain_streams[c] = lead->chain_stream[c - 1];
      LSR_HIP(hipStreamWaitEvent(chain_streams[c], lead->chain_fork_ev, 0));
    }
  }
  // launch geometry: where the leaf records are read from, which kernel, workgroup size (lead handle's tuning keys, 0 / -1 = automatic)
  NdtLaunchCfg cfg;
  cfg.batch = B;
  cfg.neighborhood = lead->ndt.neighborhood;
  choose_table_mode(lead, hs, B, cfg);
  // accumulator banks, one set per member, cleared before launch 0
  if ((st = lead->d_bins.reserve((size_t)B * NDT_NBANKS * NDT_BANK_WORDS))) return st;
  int max_blocks = 1, nb_full = 1;
  int min_evals = 1, hard_cap = 1;
  long pts = 0;
  for (int b = 0; b < B; b++) {
    lsr_handle h = hs[b];
    ndt_fill_initial_state(lead->h_state.p[2 * b], guesses ? guesses + 16 * b : nullptr, h->ndt, (int)h->source.n);
    lead->h_state.p[2 * b + 1] = lead->h_state.p[2 * b];
    fill_problem(lead->h_prob.p[b], h, lead->d_state.p + 2 * b, lead->d_bins.p + (size_t)b * NDT_NBANKS * NDT_BANK_WORDS, cfg);
    max_blocks = std::max(max_blocks, lead->h_prob.p[b].nblocks);
    nb_full = std::max(nb_full, (int)((h->source.n + cfg_wg_points(cfg) - 1) / cfg_wg_points(cfg)));
    min_evals = std::max(min_evals, ndt_min_evals(h->ndt));
    hard_cap = std::max(hard_cap, ndt_hard_cap(h->ndt));
    pts += (long)h->source.n;
  }
  cfg.max_blocks = max_blocks;
  nb_full = std::min(nb_full, NDT_MAX_BLOCKS);
  // host mailboxes, one per registration (pinned, host-coherent, mapped into the device)
  if ((size_t)B > lead->mailbox.cap) {
    LSR_HIP(hipStreamSynchronize(lead->stream));  // launches still queued from the previous align report into the old block
    if ((st = lead->mailbox.reserve((size_t)B, hipHostMallocMapped | hipHostMallocCoherent))) return st;
    std::memset(lead->mailbox.p, 0, sizeof(NdtMailbox) * lead->mailbox.cap);
    LSR_HIP(hipHostGetDevicePointer((void**)&lead->d_mailbox, lead->mailbox.p, 0));
  }
  unsigned int token = ++lead->align_token;
  if (token == 0) token = ++lead->align_token;  // 0 is the mailbox's idle value
  for (int b = 0; b < B; b++) {
    lead->h_prob.p[b].mailbox = lead->d_mailbox + b;
    lead->h_state.p[2 * b].token = lead->h_state.p[2 * b + 1].token = (int)token;
  }
  const auto t0 = std::chrono::steady_clock::now();
  // profiling brackets: a set is timed from before its state uploads (every chain does its own) to the point where the lead's stream
  // has joined every chain; a single registration from after its one-launch initialisation, as before
  if (lead->profile && B > 1) LSR_HIP(hipEventRecord(lead->ev0, lead->stream));
  if (B == 1) {  // problem and state in the kernel arguments (no SDMA copy, no memset)
    if ((st = ndt_init_single(lead->h_state.p[0], lead->d_state.p, lead->d_bins.p, lead->stream))) return st;
  } else {
    for (int c = 0; c < n_chains; c++) {   // one launch per chain: problem records + initial states out of the pinned arrays, banks cleared
      const size_t b0 = (size_t)chain_first[c], nb = (size_t)(chain_first[c + 1] - chain_first[c]);
      if ((st = ndt_init_batch(lead->h_prob_dev + b0, lead->h_state_dev + 2 * b0, lead->d_prob.p + b0, lead->d_state.p + 2 * b0,
                               lead->d_bins.p + b0 * NDT_NBANKS * NDT_BANK_WORDS, (int)nb, chain_streams[c]))) return st;
    }
  }
  if (lead->profile && B == 1) LSR_HIP(hipEventRecord(lead->ev0, lead->stream));
  // A candidate set is scored right after it is registered (graph_based_slam_component.cpp:230-231): the neighbour grids that
  // getFitnessScore needs are refined from the voxel order NOW, on a side stream, under the launch chain — the chain is a
  // sequence of short dependent launches that does not fill the chip, the refinement is one wide launch per 16 targets.
  bool prefetched = false;
  if (B > 1) {
    std::vector<const VoxelGridDev*> vgs;
    std::vector<HashGridDev*> hgs;
    std::vector<lsr_handle> owners;
    for (int b = 0; b < B; b++) {
      lsr_handle h = hs[b];
      if (!hash_from_grid_possible(h) || target_is_shared(h) || h->target->has_hash) continue;
      bool seen = false;
      for (lsr_handle o : owners) seen = seen || (o->target == h->target);
      if (seen) continue;
      vgs.push_back(&h->target->grid); hgs.push_back(&h->target->hash); owners.push_back(h);
    }
    if (!vgs.empty()) {
      LSR_HIP(hipEventRecord(lead->side_fork_ev, lead->stream));        // the targets' builds are behind this point of the lead's stream
      LSR_HIP(hipStreamWaitEvent(lead->side_stream, lead->side_fork_ev, 0));
      if ((st = nn_build_hash_from_grids(vgs.data(), hgs.data(), (int)vgs.size(), lead->side_stream))) return st;
      LSR_HIP(hipEventRecord(lead->side_ev, lead->side_stream));
      prefetched = true;
      for (lsr_handle o : owners) o->target->has_hash = true;
    }
  }
  // eager fitness: members that can be served by the group search on the side stream (their grid is there or being refined there)
  std::vector<char> eager_ok((size_t)B, 0), eager_queued((size_t)B, 0), eager_sent((size_t)B, 0);   // eligible / finished and waiting for a group / search enqueued
  std::vector<int> eager_ready;
  bool eager = false;
  if (fitness_out && B > 1) {
    for (int b = 0; b < B; b++) {
      lsr_handle h = hs[b];
      bool twice = false;
      for (int a = 0; a < b; a++) twice = twice || (hs[a] == h);
      eager_ok[b] = (!twice && hash_from_grid_possible(h) && !target_is_shared(h) && h->target->has_hash) ? 1 : 0;
      eager = eager || eager_ok[b];
    }
    if (eager && !prefetched) {   // every grid was there already: the side stream still has to start behind the lead's stream
      LSR_HIP(hipEventRecord(lead->side_fork_ev, lead->stream));
      LSR_HIP(hipStreamWaitEvent(lead->side_stream, lead->side_fork_ev, 0));
    }
  }
  const NdtMailbox* MB = lead->mailbox.p;
  auto eager_dispatch = [&](bool all) -> int {
    for (int b = 0; b < B; b++)
      if (eager_ok[b] && !eager_queued[b] && __atomic_load_n(&MB[b].done, __ATOMIC_ACQUIRE) == token) { eager_queued[b] = 1; eager_ready.push_back(b); }
    // a launch group serves up to 12 members: wait for a full group while the chain is still running.  (Round 5 measured groups of
    // ONE for small sets — a share of 8 candidates, whose chain leaves the chip idle half of the time —: a search is a wide launch
    // of long-lived waves, the chain's workgroups queue behind them for wave slots and LDS, launches of 15 us took 40-80 us, and the
    // share got slower, not faster: 0.757 / 0.949 ms against 0.710 / 0.928 ms for align + fitness of two shares.  Bounding the searches
    // and the grid refinement to 256 / 512 / 1024 resident workgroups (stride loops) so that the chain always finds its slots made it
    // worse still — 1.22 / 0.99 / 0.78 ms against 0.68 for the first share: refinement + searches are ~0.4 ms of full-chip work, at a
    // fraction of the chip they outlast the 0.5 ms chain and the tail is paid at the reduced rate.)
    constexpr size_t group = 12;
    while (!eager_ready.empty() && (all || eager_ready.size() >= group)) {
      const int n = (int)std::min(group, eager_ready.size());
      std::vector<FitJob> jobs;
      for (int k = 0; k < n; k++) {
        const int b = eager_ready[k];
        jobs.push_back(FitJob{&hs[b]->source, MB[b].final_T, &hs[b]->target->hash, max_range, &hs[b]->scratch});
      }
      const int fst = nn_fitness_begin_group(jobs.data(), n, lead->side_stream);
      if (fst) return fst;
      for (int k = 0; k < n; k++) eager_sent[eager_ready[k]] = 1;
      eager_ready.erase(eager_ready.begin(), eager_ready.begin() + n);
    }
    return LSR_OK;
  };
  const std::function<int()> poll_hook = [&]() { return eager_dispatch(false); };
  int launches = 0;
  st = run_ndt_feeder(lead, lead->d_prob.p, lead->h_prob.p, cfg, min_evals, hard_cap, token, &launches, eager ? &poll_hook : nullptr,
                      !cfg.quad ? nb_full : 0, n_chains, chain_first, chain_streams);
  // whatever follows on the lead's stream (the next align's uploads, a release of the banks) stays behind the chains' queued launches
  if (!chain_join.join() && !st) { set_last_error("joining a launch chain failed"); st = LSR_ERR_HIP; }
  if (eager && !st) st = eager_dispatch(true);
  if (eager) {
    (void)hipEventRecord(lead->side_ev, lead->side_stream);   // behind the last search
    for (int b = 0; b < B; b++) {   // every score travels through its member's host mailbox: polled, not synchronised for
      if (!eager_sent[b]) continue;
      double v = 0;
      const int fst = nn_fitness_end(hs[b]->scratch, lead->side_stream, &v);
      if (fst && !st) st = fst;
      if (!fst) fitness_out[b] = v;
    }
  }
  if (prefetched || eager) {
    // the side stream's work — grid refinement, searches — ends here: every later use of the grids and of the members' scratch
    // (any stream, any call) then needs no ordering against it (after the polls above only a kernel epilogue is left to wait for)
    if (hipEventSynchronize(lead->side_ev) != hipSuccess && !st) { set_last_error("side-stream work of the candidate set failed"); st = LSR_ERR_HIP; }
    if (st && prefetched) for (int b = 0; b < B; b++) if (hs[b]->target) hs[b]->target->has_hash = false;
  }
  if (st) return st;
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const NdtMailbox* M = lead->mailbox.p;
  if (lead->profile) {
    // hipEvents around the launch chain exactly as production runs it; the span also holds the finalising launch and
    // the (at most four) queued launches that exit at their head, so the time per pass is slightly over-estimated
    LSR_HIP(hipEventRecord(lead->ev1, lead->stream));
    LSR_HIP(hipEventSynchronize(lead->ev1));
    float ev_ms = 0.f;
    LSR_HIP(hipEventElapsedTime(&ev_ms, lead->ev0, lead->ev1));
    int passes = 0;
    lead->prof.deriv_pairs = 0;
    for (int b = 0; b < B; b++) {
      passes = std::max(passes, M[b].n_passes);   // launches that evaluated points (n_evals counts a fused pass twice)
      lead->prof.deriv_pairs += (int64_t)M[b].last_pairs;
    }
    lead->prof.deriv_ms_total += ev_ms;
    lead->prof.deriv_launches += passes;
    lead->prof.deriv_points += (int64_t)passes * pts;
  }
  for (int b = 0; b < B; b++) {
    lsr_handle h = hs[b];
    std::memcpy(h->final_T, M[b].final_T, sizeof(float) * 16);
    h->converged = M[b].converged;
    if (finals) std::memcpy(finals + 16 * b, M[b].final_T, sizeof(float) * 16);
    if (results) {
      results[b].converged = M[b].converged;
      results[b].iterations = M[b].nr_iterations;
      results[b].score = M[b].trans_probability;
      results[b].n_evaluations = M[b].n_evals;
      results[b].n_correspondences = (int)M[b].last_pairs;   // valid (point, voxel) pairs of the last derivative pass
      results[b].gpu_ms = ms;  // host clock from the state upload to the last raised flag (launches still queued are no-ops)
    }
  }
  return LSR_OK;
}

// The problem record and the table mode of a pose-scoring launch (pose_search.hip) on h's target and source: what choose_table_mode
// gives the object (LSR_NDT_TABLE_MODE included), with the LDS table only where it fits next to `other_lds` bytes of the kernel's own.
int lsr::ndt_score_problem(lsr_handle h, int other_lds, NdtProblem* P, int* tab, int* tab_bytes) {
  NdtLaunchCfg cfg;
  cfg.neighborhood = h->ndt.neighborhood;
  lsr_handle one[1] = {h};
  choose_table_mode(h, one, 1, cfg);
  const VoxelGridDev& g = h->target->grid;
  if (cfg.tab == NDT_TAB_LDS && cfg.lds_bytes + other_lds > device_lds_bytes(h->device)) cfg.tab = g.dense ? NDT_TAB_DENSE : NDT_TAB_COMPACT;
  fill_problem(*P, h, nullptr, nullptr, cfg);
  *tab = cfg.tab;
  *tab_bytes = (cfg.tab == NDT_TAB_LDS) ? g.lds_bytes : 0;
  return LSR_OK;
}

// ---- NDT inspection entries: the grid as built, one derivative pass at a given pose ---------------------------------------
extern "C" {

int lsr_ndt_grid_info(lsr_handle h, int32_t* info8) {
  LSR_CHECK_HANDLE(h);
  if (!info8) return LSR_ERR_INVALID_ARGUMENT;
  if (!h->target) return LSR_ERR_NO_TARGET;
  int st = ensure_ndt_grid(h);
  if (st) return st;
  const VoxelGridDev& g = h->target->grid;
  std::vector<int> keys(g.n_leaves);
  if (g.n_leaves) LSR_HIP(hipMemcpy(keys.data(), g.leaf_key.p, sizeof(int) * g.n_leaves, hipMemcpyDeviceToHost));
  int real = 0;
  for (int k : keys) real += (k >= 0);
  for (int k = 0; k < 3; k++) { info8[k] = g.min_b[k]; info8[3 + k] = g.max_b[k]; }
  info8[6] = real;
  info8[7] = g.n_valid;
  return LSR_OK;
}

int lsr_ndt_grid_dump(lsr_handle h, int32_t* idx, int32_t* npts, double* mean, double* icov) {
  LSR_CHECK_HANDLE(h);
  if (!h->target) return LSR_ERR_NO_TARGET;
  int st = ensure_ndt_grid(h);
  if (st) return st;
  const VoxelGridDev& g = h->target->grid;
  const int L = g.n_leaves;
  if (L == 0) return LSR_OK;
  std::vector<int> keys(L), cnt(L);
  std::vector<double> m((size_t)L * 3), ic((size_t)L * 9);
  LSR_HIP(hipMemcpy(keys.data(), g.leaf_key.p, sizeof(int) * L, hipMemcpyDeviceToHost));
  LSR_HIP(hipMemcpy(cnt.data(), g.leaf_n.p, sizeof(int) * L, hipMemcpyDeviceToHost));
  LSR_HIP(hipMemcpy(m.data(), g.mean64.p, sizeof(double) * L * 3, hipMemcpyDeviceToHost));
  LSR_HIP(hipMemcpy(ic.data(), g.icov64.p, sizeof(double) * L * 9, hipMemcpyDeviceToHost));
  // leaves are already in ascending key order (radix sort); the non-finite sentinel run has key -1
  int c = 0;
  for (int r = 0; r < L; r++) {
    if (keys[r] < 0) continue;
    idx[c] = keys[r];
    npts[c] = cnt[r];
    for (int k = 0; k < 3; k++) mean[c * 3 + k] = m[(size_t)r * 3 + k];
    for (int k = 0; k < 9; k++) icov[c * 9 + k] = ic[(size_t)r * 9 + k];
    c++;
  }
  return LSR_OK;
}

int lsr_ndt_grid_centroids(lsr_handle h, float* centroid) {
  LSR_CHECK_HANDLE(h);
  if (!centroid) return LSR_ERR_INVALID_ARGUMENT;
  if (!h->target) return LSR_ERR_NO_TARGET;
  int st = ensure_ndt_grid(h);
  if (st) return st;
  TargetData& t = *h->target;
  {
    std::lock_guard<std::mutex> lock(t.build_mutex);
    if (!t.has_centroids && t.grid.ncells > 0) {
      if ((st = ndt_build_centroids(t.cloud, t.grid, h->scratch, h->stream))) return st;
      t.has_centroids = true;
    }
  }
  const VoxelGridDev& g = t.grid;
  const int L = g.n_leaves;
  if (L == 0) return LSR_OK;
  const size_t n_slots = g.dense ? g.ncells : (size_t)L;
  std::vector<int> keys(L), slot(g.ncells);
  std::vector<float> cen(n_slots * 4);
  LSR_HIP(hipMemcpy(keys.data(), g.leaf_key.p, sizeof(int) * L, hipMemcpyDeviceToHost));
  LSR_HIP(hipMemcpy(slot.data(), g.cell_slot.p, sizeof(int) * g.ncells, hipMemcpyDeviceToHost));
  LSR_HIP(hipMemcpy(cen.data(), g.centroid.p, sizeof(float) * 4 * n_slots, hipMemcpyDeviceToHost));
  int c = 0;
  for (int r = 0; r < L; r++) {
    if (keys[r] < 0) continue;
    const int s = kd_slot(slot[(size_t)keys[r]]);
    for (int k = 0; k < 3; k++) centroid[c * 3 + k] = (s >= 0) ? cen[(size_t)s * 4 + k] : std::numeric_limits<float>::quiet_NaN();
    c++;
  }
  return LSR_OK;
}

int lsr_ndt_derivatives(lsr_handle h, const double* p6, const float* T16, int compute_hessian, double* score, double* grad,
                        double* hess) {
  return lsr_ndt_derivatives_pairs(h, p6, T16, compute_hessian, score, grad, hess, nullptr);
}

int lsr_ndt_derivatives_pairs(lsr_handle h, const double* p6, const float* T16, int compute_hessian, double* score, double* grad,
                              double* hess, double* pairs) {
  LSR_CHECK_HANDLE(h);
  if (!p6 || compute_hessian < 0 || compute_hessian > 2) return LSR_ERR_INVALID_ARGUMENT;
  if (!h->target || h->target->n == 0) return LSR_ERR_NO_TARGET;
  if (!h->has_source) return LSR_ERR_NO_SOURCE;
  int st = ensure_ndt_grid(h);
  if (st) return st;
  if (h->target->grid.ncells == 0) { set_last_error("the input target holds no finite point"); return LSR_ERR_NO_TARGET; }
  if ((st = h->d_state.reserve(2))) return st;
  if ((st = h->h_state.reserve(2, hipHostMallocMapped))) return st;
  if ((st = h->d_prob.reserve(1))) return st;
  if ((st = h->h_prob.reserve(1, hipHostMallocMapped))) return st;
  NdtLaunchCfg cfg;
  cfg.neighborhood = h->ndt.neighborhood;
  {
    lsr_handle one[1] = {h};
    choose_table_mode(h, one, 1, cfg);
  }
  if ((st = h->d_bins.reserve((size_t)NDT_NBANKS * NDT_BANK_WORDS))) return st;
  LSR_HIP(hipMemsetAsync(h->d_bins.p, 0, sizeof(long long) * NDT_NBANKS * NDT_BANK_WORDS, h->stream));
  cfg.max_blocks = ndt_nblocks(h->source.n, h->device, 1, cfg_wg_threads(cfg), cfg_wg_points(cfg));
  ndt_fill_diag_state(h->h_state.p[0], p6, T16, compute_hessian, h->ndt, (int)h->source.n);
  h->h_state.p[1] = h->h_state.p[0];
  fill_problem(h->h_prob.p[0], h, h->d_state.p, h->d_bins.p, cfg);
  LSR_HIP(hipMemcpyAsync(h->d_prob.p, h->h_prob.p, sizeof(NdtProblem), hipMemcpyHostToDevice, h->stream));
  LSR_HIP(hipMemcpyAsync(h->d_state.p, h->h_state.p, 2 * sizeof(NdtState), hipMemcpyHostToDevice, h->stream));
  // launch 0 evaluates, launch 1 folds the bank into the state (PH_DIAG) -> state buffer (2 & 1) = 0
  if ((st = ndt_launch_evals(h->d_prob.p, h->h_prob.p, cfg, 0, 2, h->stream))) return st;
  LSR_HIP(hipMemcpyAsync(h->h_state.p, h->d_state.p, sizeof(NdtState), hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  const NdtState& S = h->h_state.p[0];
  if (score) *score = S.score;
  if (grad) for (int i = 0; i < 6; i++) grad[i] = S.g[i];
  if (hess) for (int i = 0; i < 36; i++) hess[i] = compute_hessian ? S.H[i] : 0.0;
  if (pairs) *pairs = S.last_pairs;
  return LSR_OK;
}

}  // extern "C"
