// rec_plan.cpp -- which persistent kernel runs a layer's time recurrence, and its launch: the host side of lstm_persistent.hip.
// ONE selection function per pass (lstm_fwd_plan / lstm_bwd_plan) decides the instantiation -- a row of the kernel file's table
// (rec_kernels.h) -- its grid and windows, and states everything a caller has to know; the launchers execute the plan they are given.
#include "rec_kernels.h"

#include <atomic>
#include <map>
#include <mutex>
#include <tuple>

namespace eesen {
namespace {

constexpr int NW = kRecWaves;

// EESEN_GPU_SHARE=n (tuning.h): this process may count on 1/n of the device's CUs -- n trainer processes on one GPU (the reference's
// own two-jobs-one-GPU test mode; tests/test_gpu_multirank.py) each size their persistent grids against their share, so that all
// of them are co-resident TOGETHER instead of relying on the spin time-outs to find out that they are not.
// (round 6: a communicator that finds several of its ranks on ONE device sets the share itself -- set_gpu_share, comm.cpp -- so that
// co-located trainer jobs need no environment variable; an explicit EESEN_GPU_SHARE wins)
std::atomic<int> g_share_override{0};
int gpu_share() {
  static const int env = [] { const char* e = getenv("EESEN_GPU_SHARE"); const int v = e && *e ? atoi(e) : 0; return v < 1 ? 0 : v; }();
  if (env) return env;
  const int o = g_share_override.load(std::memory_order_relaxed);
  return o > 0 ? o : 1;
}
// the CUs this process sizes its tiles and grids against: the device's, divided by EESEN_GPU_SHARE
int share_of_cus() {
  int ncu = 256, dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  return std::max(1, ncu / gpu_share());
}

// (see "The persistent grids are launched as ORDINARY kernels" below)
template <class... Args>
void plan_launch(hipStream_t st, const void* fn, int wgs, Args... args) {
  void* argv[] = {static_cast<void*>(&args)...};
  EESEN_HIP_CHECK(hipLaunchKernel(fn, dim3(wgs), dim3(NW * 64), argv, 0, st));
}

// Residency census of one instantiation of the bf16-pipe kernel: `wgs` workgroups launched in its census mode (T < 0) on the idle
// device must all check in within 5 ms.  Once per (device, instantiation, workgroup count) and process, ~1 ms; the occupancy query's
// own number is only trusted where this has seen it (the MI355X guide: the query over-reports by one block per CU for SGPR-heavy kernels).
bool bf_census(const RecKernel& k, int wgs) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, int>, bool> seen;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  // A device this process SHARES (EESEN_GPU_SHARE > 1: peers' grids come and go) has no idle moment to take a census in, and its
  // answer would differ from rank to rank and run to run -- and with it the forward tile, whose two candidates are not bit-identical
  // (ADVICE r5): there the occupancy query's margin decides alone, the same way in every process.
  if (gpu_share() > 1) return false;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(dev, k.fn, wgs);
  if (auto it = seen.find(key); it != seen.end()) return it->second;
  bool ok = false;
  unsigned* w = nullptr;
  if (hipDeviceSynchronize() == hipSuccess && hipMalloc(reinterpret_cast<void**>(&w), 2 * sizeof(unsigned)) == hipSuccess) {
    // up to three takes: a grid that fits an idle device is seen at once; one transient occupant (another stream's kernel retiring)
    // must not decide the tile for the life of the process
    for (int take = 0; take < 3 && !ok; ++take) {
      if (hipMemset(w, 0, 2 * sizeof(unsigned)) != hipSuccess) break;
      LstmLayerDev L{};
      L.T = -1;
      unsigned* err = w + 1;
      int spin_limit = 0;
      unsigned long long* trace = nullptr;
      RecRole role{1, 1, 1, 0};
      void* argv[] = {&L, &w, &err, &spin_limit, &trace, &role};
      if (hipLaunchKernel(k.fn, dim3(wgs), dim3(NW * 64), argv, 0, nullptr) != hipSuccess) { (void)hipGetLastError(); break; }
      unsigned e = 1;
      ok = hipMemcpy(&e, w + 1, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess && e == 0;
    }
    (void)hipFree(w);
  }
  seen[key] = ok;
  if (getenv("EESEN_PRINT_PLAN")) fprintf(stderr, "LOG (eesen_hip) residency census: %d workgroups of %s on device %d: %s\n", wgs, k.name, dev, ok ? "seen co-resident" : "NOT seen");
  return ok;
}

// census: this instantiation has a residency census (bf_census): have the grid's workgroups been SEEN co-resident on this device?
bool fits(const RecKernel& k, dim3 grid, bool census = false) {  // grid: the workgroups of ONE launch (one sequence window)
  int dev = 0, ncu = 0, nb = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  {  // the occupancy of an instantiation does not change: asked once per (device, kernel) -- this runs several times per plan
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> cache;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, k.fn);
    auto it = cache.find(key);
    if (it == cache.end()) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, NW * 64, 0) != hipSuccess) return false;
      it = cache.emplace(key, nb).first;
    }
    nb = it->second;
  }
  // the occupancy query can over-report by one workgroup per CU (MI355X guide: SGPR-heavy kernels): keep a margin of one -- unless the
  // caller has a residency CENSUS for this instantiation, which settles whether the query's own number is real
  const long wgs = (long)grid.x * grid.y * grid.z;
  if (wgs <= (long)ncu * std::max(1, nb - 1) / gpu_share()) return true;
  return census && wgs <= (long)ncu * nb / gpu_share() && bf_census(k, (int)wgs);
}

// The persistent grids are launched as ORDINARY kernels: hipLaunchCooperativeKernel costs ~40 us more per launch (its dedicated
// queue; 0.3 ms per cfg2 step over eight launches, measured) and guarantees nothing that fits() has not checked already -- the
// runtime does not gang-schedule a cooperative grid either (the side-stream GEMMs co-run with it), it only refuses grids above the
// occupancy limit, which is the check fits() makes with a workgroup per CU of margin.  Workgroups that are not resident at once
// are waited for by the others' bounded spins, and a spin that gives up is recovered from (net.cpp).

// Counter words one launch clears: `groups` (direction, sequence tile) groups -- x 4 K quarters on the K-split tiles -- of kShards
// shards, a 128-byte line each.  A pass has kCtlHalf of them.
size_t ctl_words(size_t groups) { return groups * kShards * kShardStride; }

// The hand-off relies on every step reading cache lines nobody has touched before in this launch.  That holds only if
// a time step's row block [S x cols] (Y forward, DG backward; a sequence window's rows likewise) starts on a 128-byte line:
// otherwise the last line of block t also carries the first bytes of block t+1, gets cached (L1 and the XCD's non-coherent L2)
// while block t+1 is still unwritten, and is read back stale one step later (seen at S = 17, H = 20).  Such shapes use the
// per-step kernels.
bool line_aligned(int seqs, int cols) { return ((size_t)seqs * cols * sizeof(float)) % 128 == 0; }

// Sequence windows: the smallest number of equal windows (each a multiple of the sequence tile) whose workgroups can all be
// co-resident.  1 for every configuration but the largest (S = 64 at H = 1024 needs 512 workgroups of the wide tiles: two
// windows of 32 sequences, run one after the other -- the sequences are independent chains).
template <class F>
int pick_windows(int S, int seq_tile, F fits_with) {
  for (int nwin = 1; nwin <= 8; nwin *= 2) {
    if (S % nwin != 0 || (S / nwin) % seq_tile != 0) { if (nwin == 1 && fits_with(S)) return 1; continue; }
    if (fits_with(S / nwin)) return nwin;
  }
  return 0;
}

// The plan takes row `k` on `grid`: kind and name from the row, registers and LDS of the instantiation, and what its grid leaves
// free on a CU (RecPlan::free_vgprs): a SIMD has 512 registers per lane, allocated in blocks of 8; a 512-thread workgroup is two
// waves per SIMD.  `words`: ctl_words of one launch.
void take(RecPlan& P, const RecKernel& k, const dim3& grid, size_t words, int seq_tile, int units, int windows) {
  P.kind = k.kind; P.fn = k.fn; P.kernel = k.name;
  P.seq_tile = seq_tile; P.units = units; P.windows = windows; P.ctl_words = words;
  P.grid[0] = (int)grid.x; P.grid[1] = (int)grid.y; P.grid[2] = (int)grid.z;
  P.wgs = (int)(grid.x * grid.y * grid.z);
  P.wgs_per_cu = std::max(1, cdiv(P.wgs, share_of_cus()));
  static std::mutex mu;
  static std::map<const void*, std::pair<int, int>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(P.fn);
  if (it == cache.end()) {
    hipFuncAttributes a{};
    if (hipFuncGetAttributes(&a, P.fn) != hipSuccess) { (void)hipGetLastError(); return; }
    it = cache.emplace(P.fn, std::make_pair((int)a.numRegs, (int)a.sharedSizeBytes)).first;
  }
  P.vgprs = it->second.first;
  P.lds = it->second.second;
  if (P.vgprs > 0) P.free_vgprs = 512 - P.wgs_per_cu * (NW / 4) * ((P.vgprs + 7) & ~7);
}

// ---- forward: tile and instantiation ----------------------------------------------------------------------------------------
// Forward tile (sequences x hidden units per workgroup), chosen so that every CU gets ONE workgroup where the shape allows:
//   32 x 4  <MT=2, NT=1>: the decomposition of lstm_fwd_step_kernel (any H)
//   16 x 8  <MT=1, NT=2>: half the m_{t-1} fetch per CU; 256 workgroups at H = 512, S = 32
//   16 x 16 <MT=1, NT=4>: for wide layers (H = 1024: 16 x 8 would need 512 co-resident workgroups); 64 gate rows of W_m
//                         (256 KB at H = 1024) live in the registers of one workgroup
struct FwdTile { int mt, nt; };
// Which instantiation of lstm_fwd_persistent_bf_kernel, if any, this layer's forward recurrence takes (bf_plan_shape)
struct BfPlan { bool on; int cpw, nt, ap, wp; bool f16; };

bool small_xchg(const LstmLayerDev& L, int bytes_per_unit_row) {   // block offsets of the exchange buffer within 32 bits
  return (size_t)L.T * L.ndir * cdiv(L.S, 16) * (size_t)(L.H / 32) * bytes_per_unit_row < ((size_t)1 << 31);
}
bool bf_fits(const LstmLayerDev& L, const BfPlan& P, int Sw) {
  const RecKernel* k = rec_kernel(kFwdBf, P.cpw, P.nt, P.ap, P.wp, P.f16);
  return k && fits(*k, dim3(L.H / (4 * P.nt), L.ndir, cdiv(Sw, 16)), /* census */ true);
}
// the narrow bf16-pipe tile as up to two workgroups per CU (fwd_tile): the plan's own shape conditions, and the grid seen co-resident
bool narrow2_ok(const LstmLayerDev& L, int need) {
  const bool f16 = L.fwd_f16 && L.wm_amax != nullptr;
  if (!L.fwd_narrow2 || !(L.fwd_split || f16) || L.fwd_bf16 || L.X == nullptr || L.drop_mode || L.T < 2 || L.H % 32 != 0) return false;
  if (!small_xchg(L, 1024 * 3)) return false;
  return bf_fits(L, f16 ? BfPlan{true, need, 2, 2, 2, true} : BfPlan{true, need, 2, 3, 3, false}, L.S);
}
FwdTile fwd_tile(const LstmLayerDev& L) {
  const int need = ((L.H + 31) / 32 + NW - 1) / NW;
  const int ncu = share_of_cus();
  // (wide layers take the 16-sequence tile at ANY batch size: their 32 x 4 tile would need H/4 x ndir workgroups -- 512 at H = 1024 --
  // and a batch of <= 16 sequences fell back to the per-step kernels: seen at S = 16, T = 3000 with the six-layer cfg5 stack, round 4)
  // (S <= 16 on narrow layers: the 32 x 4 tile has twice the workgroups of the 16 x 8 tile -- but only the latter has the bf16-pipe
  // kernel; LstmLayerDev::fwd_t16_small takes it there too where that kernel applies)
  const bool t16_ok = L.H % 8 == 0 && (L.S > 16 || need > 2 || (L.fwd_t16_small && L.fwd_split && !L.drop_mode && L.X && L.H % 32 == 0));
  // The narrow 16 x 8 tile needs H/8 x ndir x S/16 workgroups: one per CU up to S = 32 at H = 512.  Beyond that, up to TWO per CU
  // (round 5; S = 64 at H = 512: 512 workgroups of the bf16-pipe kernel, 108 registers) where a residency census has SEEN that many
  // co-resident (narrow2_ok) -- two chains per CU interleaved by the hardware: 3.5 us per step for 64 sequences against 4.2 on the
  // wide tile; otherwise the wide 16 x 16 tile.
  const long narrow_wgs = (long)(L.H / 8) * L.ndir * cdiv(L.S, 16);
  const bool narrow_full = narrow_wgs > ncu && !(narrow_wgs <= 2L * ncu && need <= 2 && narrow2_ok(L, need));
  if (t16_ok && L.H % 16 == 0 && need <= 4 && (need > 2 || narrow_full)) return {1, 4};
  if (t16_ok && need <= 2) return {1, 2};
  return {2, 1};
}

// Which instantiation of lstm_fwd_persistent_bf_kernel the shape and the switches ask for (whether its grid is co-resident: lstm_fwd_plan):
//   * BASELINE config 4's bf16 forward (L.fwd_bf16: W_m as hi + lo planes, m_t one plane): the wide tile's
//     geometry (16 sequences x 16 units), whole 256-unit multiples (each of the 8 waves owns CPW = H / 256 chunks of 32 units);
//   * the fp32-class 3-way split (L.fwd_split; three planes each): wherever the narrow 16 x 8 fp32 tile would be taken.
// Both: exchange buffer present, no recurrent dropout, block offsets within 32 bits.
//   * round 6, fp32-class on two fp16 planes per operand (L.fwd_f16 and the layer's W_m bound on hand): the narrow tile like the
//     3-way split, AND the wide 16 x 16 tile (whole 256-unit multiples) that had only the fp32-input kernel.
BfPlan bf_plan_shape(const LstmLayerDev& L, const FwdTile& ft) {
  const BfPlan off{false, 0, 0, 0, 0, false};
  if (L.X == nullptr || L.drop_mode || L.T < 2 || L.H % 32 != 0) return off;
  if (L.fwd_bf16) {
    if (L.H % 256 != 0 || L.H / 256 > 4 || !small_xchg(L, 1024)) return off;
    return {true, L.H / 256, 4, 1, 2, false};
  }
  const bool f16 = L.fwd_f16 && L.wm_amax != nullptr;
  if (L.fwd_split || f16) {
    const int need = (L.H / 32 + NW - 1) / NW;
    if (f16 && ft.mt == 1 && ft.nt == 4 && L.H % 256 == 0 && L.H / 256 <= 4 && small_xchg(L, 1024 * 2)) return {true, L.H / 256, 4, 2, 2, true};
    if (ft.mt != 1 || ft.nt != 2 || need > 2 || L.H % 8 != 0 || !small_xchg(L, 1024 * 3)) return off;
    if (f16) return {true, need, 2, 2, 2, true};
    if (L.fwd_split) return {true, need, 2, 3, 3, false};
  }
  return off;
}

// the K-split backward tiles apply to this shape (wide layers without dropout, wherever the 16-sequence tile would be taken: narrow
// layers take the 4 x 32 tile, dropout layers and odd shapes the generic one).  LstmLayerDev::bwd_ksplit = 0 (EESEN_BWD_KSPLIT=0)
// switches them off.
bool bwd_ksplit_shape(const LstmLayerDev& L, int stile) {
  return L.bwd_ksplit && stile == 16 && !L.drop_mode && L.H % 256 == 0 && L.H >= 768 && L.H <= 1024 && L.T >= 2;
}
// ... and their fp16-plane form (shape and switches)
bool bwd_planes_shape(const LstmLayerDev& L, int stile) {
  const int cpw = L.H / (32 * NW);
  return L.bwd_f16 && L.wm_amax != nullptr && bwd_ksplit_shape(L, stile) && (cpw == 2 || cpw == 4) && L.H % (32 * NW) == 0;
}

}  // namespace

void set_gpu_share(int n) { g_share_override.store(n < 1 ? 1 : n, std::memory_order_relaxed); }
int gpu_share_value() { return gpu_share(); }

// One-way flight of an agent-scope increment between two CUs of the current device, in nanoseconds (measured once per device and
// process, ~3 ms: 2000 round trips, the median of five runs).  The first-poll delays of the recurrence kernels are multiples of it.
float handoff_flight_ns() {
  static float cache[64] = {0};
  static std::mutex mu;                       // Nets may be created from several host threads
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0.f;
  if (cache[dev] > 0.f) return cache[dev];
  unsigned* flags = nullptr;
  unsigned long long* out = nullptr;
  EESEN_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&flags), 64 * sizeof(unsigned)));
  EESEN_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&out), sizeof(unsigned long long)));
  int rounds = 2000;
  double ns[5];
  for (int rep = 0; rep < 5; ++rep) {
    EESEN_HIP_CHECK(hipMemset(flags, 0, 64 * sizeof(unsigned)));
    void* argv[] = {&flags, &out, &rounds};
    (void)hipLaunchKernel(handoff_pingpong_fn(), dim3(2), dim3(64), argv, 0, nullptr);
    unsigned long long ticks = 0;
    EESEN_HIP_CHECK(hipMemcpy(&ticks, out, sizeof(ticks), hipMemcpyDeviceToHost));
    // 0 ticks: the two workgroups never saw each other (not co-resident on a busy device): no measurement, the default flight
    ns[rep] = ticks ? 10.0 * (double)ticks / (2.0 * rounds) : 500.0;
  }
  std::sort(ns, ns + 5);
  (void)hipFree(flags);
  (void)hipFree(out);
  // (the median of five.  The measurement has two modes on an MI355X -- 370-420 ns and 550-620 ns, by where the dispatcher puts the two
  // workgroups; some boxes read the far one every time -- and a step's time does not depend on which one its process measured: net.cpp
  // uses the delays tuned on this part whenever the reading is in that range, and the reading itself only as a plausibility check)
  cache[dev] = (float)std::min(2000.0, std::max(100.0, ns[2]));
  return cache[dev];
}

void wait_for_word(hipStream_t st, const unsigned* word, unsigned target, unsigned* err, double limit_s) {
  unsigned long long ticks = (unsigned long long)(std::max(0.05, limit_s) * 1e8);   // wall_clock64: 100 MHz
  void* argv[] = {&word, &target, &err, &ticks};
  (void)hipLaunchKernel(wait_for_word_fn(), dim3(1), dim3(64), argv, 0, st);
  check_launch("wait_for_word");
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// ctl: [0 .. 2*ndir*nz) arrival counters (fwd then bwd use disjoint halves via `ctl_off`), last word = error flag
RecPlan lstm_fwd_plan(const LstmLayerDev& L) {
  RecPlan P;
  const int need = ((L.H + 31) / 32 + NW - 1) / NW;
  const FwdTile ft = fwd_tile(L);
  if (need > 4 || (ft.nt == 2 && need > 2) || L.H % (4 * ft.nt) != 0 || L.T < 2) return P;
  if (!line_aligned(L.S, L.ndir * L.H)) return P;
  if ((size_t)(L.T + 2) * L.S * L.ndir * L.H * sizeof(float) >= ((size_t)1 << 31)) return P;  // 32-bit buffer offsets over all of Y
  // On the bf16 matrix pipe (config 4's bf16 forward, the fp32-class 3-way split or two fp16 planes) where the shape asks for it and
  // the instantiation's workgroups are co-resident in SOME number of sequence windows: a shape or device on which only the bf16-pipe
  // tile does not fit falls through to the fp32 tiles (which ran in this slot before round 4) instead of dropping to the
  // one-launch-per-step kernels.
  BfPlan B = bf_plan_shape(L, ft);
  const bool drop = L.drop_mode != 0;
  const int cpw32 = ft.nt == 2 ? std::min(need, 2) : need <= 2 ? need : 4;   // chunks per wave of the fp32 tiles' instantiations
  int nwin = B.on ? pick_windows(L.S, 16, [&](int Sw) { return bf_fits(L, B, Sw); }) : 0;
  if (nwin == 0) {
    B.on = false;
    // (co-residency of the fp32 tile is asked of its plain-fetch instantiation, whichever fetch the launch takes)
    const RecKernel* probe = rec_kernel(kFwdF32, cpw32, ft.mt, ft.nt, drop, false);
    nwin = pick_windows(L.S, 16 * ft.mt, [&](int Sw) { return probe && fits(*probe, dim3(L.H / (4 * ft.nt), L.ndir, cdiv(Sw, 16 * ft.mt))); });
  }
  if (nwin == 0) return P;
  if (nwin > 1 && !line_aligned(L.S / nwin, L.ndir * L.H)) return P;
  const int mt = B.on ? 1 : ft.mt, nt = B.on ? B.nt : ft.nt, nz = cdiv(L.S, 16 * mt);   // nz: sequence tiles over the whole batch
  auto answer = [&](const RecKernel& k, const dim3& grid, size_t words, int seq_tile, int windows, bool one_window) {
    take(P, k, grid, words, seq_tile, 4 * nt, windows);
    P.seq_tiles = nz;
    P.one_window = one_window;
    // room for a 128 x 128 GEMM workgroup on the same CU: the narrow tiles (<= 8 units, <= 131 VGPRs); the wide fp32 tile (206 VGPRs)
    // does not (the bf16 forward's successor in BASELINE config 4 is a projection, not an LSTM layer; two narrow workgroups per CU
    // leave no room)
    P.leaves_room = nt <= 2 && (!B.on || (long)(L.H / (4 * nt)) * L.ndir * nz <= share_of_cus());
    P.bf16 = L.fwd_bf16 && k.kind == kRecFwdBf;
  };
  const dim3 grid(L.H / (4 * nt), L.ndir, cdiv(L.S / nwin, 16 * mt));
  const size_t words = ctl_words(grid.y * grid.z);
  if (B.on) {
    if (words <= (size_t)kCtlHalf) {
      answer(*rec_kernel(kFwdBf, B.cpw, B.nt, B.ap, B.wp, B.f16), grid, words, 16, nwin, nwin == 1);
      if (const RecKernel* g = rec_kernel(kFwdBfGuard, B.cpw, B.nt, B.ap, B.wp, B.f16)) P.fn_guard = g->fn;   // (same tile, same footprint class)
    }
    return P;
  }
  // exchange-layout operand fetch: 16-sequence tiles, whole 32-unit chunks, block offsets within 32 bits
  const bool xchg = L.X != nullptr && ft.mt == 1 && L.H % 32 == 0 && !drop && small_xchg(L, 2048);
  // Two windows of the wide tile: one launch that time-multiplexes the two sequence tiles of every workgroup instead
  // (lstm_fwd_persistent_mux_kernel).  LstmLayerDev::fwd_mux = 0 (EESEN_FWD_MUX=0): the two launches, one after the other.
  if (L.fwd_mux && nwin == 2 && ft.mt == 1 && ft.nt == 4 && need > 2 && need <= 4 && !drop && L.H % 32 == 0) {
    const RecKernel& k = *rec_kernel(kFwdMux, 4, 4, xchg);
    const dim3 mgrid(L.H / 16, L.ndir, cdiv(nz, 2));
    if (fits(k, mgrid) && ctl_words((size_t)L.ndir * nz) <= (size_t)kCtlHalf) {   // (its counters cover every tile of the batch)
      answer(k, mgrid, ctl_words((size_t)L.ndir * nz), 32, 1, false);
      return P;
    }
  }
  if (words > (size_t)kCtlHalf) return P;
  const RecKernel* k = rec_kernel(kFwdF32, cpw32, ft.mt, ft.nt, drop, xchg);
  EESEN_REQUIRE(k != nullptr, EESEN_ERR_STATE, "no instantiation of the fp32 forward tile for this plan");
  answer(*k, grid, words, 16 * ft.mt, nwin, nwin == 1);
  return P;
}

void lstm_fwd_launch(hipStream_t st, const RecPlan& P, const LstmLayerDev& L0, unsigned* cnt, unsigned* err, int spin_limit,
                     unsigned long long* trace, hipEvent_t after_reset) {
  EESEN_REQUIRE(P.kind == kRecFwdBf || P.kind == kRecFwdMux || P.kind == kRecFwdF32, EESEN_ERR_STATE, "not a forward recurrence plan");
  const RecRole role{P.grid[0], P.grid[1], P.grid[2], L0.xcd_map};
  for (int w = 0; w < P.windows; ++w) {
    LstmLayerDev L = L0;
    if (P.kind == kRecFwdMux) { L.s_begin = 0; L.s_count = 0; }
    else { L.s_count = L0.S / P.windows; L.s_begin = w * L.s_count; }
    // Two workgroups per CU (the narrow tile at --num-sequence 64): a step takes a quarter longer and its increments land later -- the
    // first poll 700 ns after the publish instead of 400.  Swept on the final kernels (round 6, cfg2 at S = 64, ms per step at a first
    // poll after 300 / 400 / 500 / 600 / 700 / 850 ns: 52.8 / 52.0 / 51.0-51.7 / 51.4 / 51.0 / 51.4; profiles/r06_poll_sweep.log).
    if (P.kind != kRecFwdMux && P.wgs_per_cu >= 2 && !L0.poll_raw) L.poll_delay = L0.poll_delay * 7 / 4;
    EESEN_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned) * P.ctl_words, st));
    if (after_reset && P.one_window) EESEN_HIP_CHECK(hipEventRecord(after_reset, st));  // a gated consumer may start polling from here on
    if (P.kind == kRecFwdMux) plan_launch(st, P.fn, P.wgs, L, cnt, err, spin_limit, role);
    else {
      const bool guarded = L.guard[0] != nullptr || L.guard[1] != nullptr;
      EESEN_REQUIRE(!guarded || P.fn_guard, EESEN_ERR_STATE, "row guards set for a forward plan without a guarded instantiation");
      plan_launch(st, guarded ? P.fn_guard : P.fn, P.wgs, L, cnt, err, spin_limit, trace, role);
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
RecPlan lstm_bwd_plan(const LstmLayerDev& L) {
  RecPlan P;
  const int need = ((4 * L.H + 31) / 32 + NW - 1) / NW;
  const int ldG = L.ndir * 4 * L.H;
  // Sequences per workgroup: 16 fills the MFMA rows; 8 wastes half of them but halves the 128 KB of DG_next each workgroup
  // must fetch per step, which is what bounds the step (measured: 3.75 us of fetch at ~34 GB/s per CU vs 1.8 us of MFMA).
  // Take 8 whenever 16 would leave half of the chip's CUs without a workgroup.
  const long blocks16 = (long)cdiv(L.H, 16) * L.ndir * cdiv(L.S, 16);
  const int stile = 2 * blocks16 <= share_of_cus() && L.S > 8 ? 8 : 16;
  P.light = stile == 8;   // (a property of the SHAPE: it also holds for the per-step kernels a shape without a persistent tile takes)
  if (need > 16 || L.T < 2) return P;
  if (!line_aligned(L.S, ldG)) return P;
  // 32-bit buffer offsets: the kernel re-bases its DG resource every `chunk` steps; a chunk touches chunk + 1 row blocks
  const size_t blk_bytes = (size_t)L.S * ldG * sizeof(float);
  const long max_blocks = (long)((((size_t)1 << 31) - 1) / blk_bytes);
  if (max_blocks < 3) return P;
  int chunk = (int)std::min<long>(L.T, max_blocks - 1);
  if (chunk < L.T) { int p2 = 1; while (p2 * 2 <= chunk) p2 *= 2; chunk = p2; }   // a power of two keeps `step % chunk` cheap
  P.chunk = chunk;
  // `k` in the smallest number of sequence windows that are co-resident, line-aligned and within the pass's counters (`quarters`:
  // counter sets per group); false: in none
  auto in_windows = [&](const RecKernel* k, int gx, int seq_tile, int units, int quarters) {
    if (!k) return false;
    auto grid_of = [&](int Sw) { return dim3(gx, L.ndir, cdiv(Sw, seq_tile)); };
    auto words_of = [&](const dim3& g) { return ctl_words((size_t)g.y * g.z * quarters); };
    const int nwin = pick_windows(L.S, seq_tile, [&](int Sw) { return words_of(grid_of(Sw)) <= (size_t)kCtlHalf && fits(*k, grid_of(Sw)); });
    if (nwin == 0 || (nwin > 1 && !line_aligned(L.S / nwin, ldG))) return false;
    take(P, *k, grid_of(L.S / nwin), words_of(grid_of(L.S / nwin)), seq_tile, units, nwin);
    return true;
  };
  // The 4-sequence x 32-unit tile (lstm_bwd_persistent_q4_kernel<., 4>): wherever the 8-sequence tile would be taken and the shape
  // allows; with TWO 4-sequence tiles per workgroup (<., 8>, round 5) where that grid does not fit but half as many workgroups do
  // (S = 64 at H = 512) -- LstmLayerDev::bwd_q4_st8: 0 = never (the 16 x 16 tile there, as before round 5), 2 = wherever it applies,
  // before the one-tile form (the tests' A/B arm: same gate gradients bit for bit)
  for (int pass = 0; pass < 2; ++pass) {
    const int stq = (L.bwd_q4_st8 == 2) == (pass == 0) ? 8 : 4;
    // (round 5: any whole number of 32-unit workgroups up to 512 cells -- the recipes' 320 among them: the waves' k chunks beyond 4H read
    // as zero and their weights ARE zero, so K = 4H need not fill the 8 waves x CPW / 2 pairs exactly)
    if (!L.bwd_q4 || L.drop_mode || L.H % 32 != 0 || L.H > 512 || chunk < L.T) break;
    // (a ragged last tile is masked in the kernel -- operand rows and cells beyond S -- so S need not be a multiple of the tile: the
    // recipes' default --num-sequence 10 takes this tile too)
    if (stq == 4 && stile != 8) continue;
    if (stq == 8 && !(L.bwd_q4_st8 && L.S > 8)) continue;
    const int cpw = 2 * ((L.H + 127) / 128);   // 2, 4, 6 or 8 chunks of 32 floats per wave: K = 4H in 8 waves x (cpw / 2) pairs of 64
    const dim3 grid(L.H / 32, L.ndir, cdiv(L.S, stq));
    const size_t words = ctl_words((size_t)grid.y * grid.z);
    const RecKernel& k = *rec_kernel(kBwdQ4, cpw, stq);
    if (fits(k, grid) && words <= (size_t)kCtlHalf) {
      take(P, k, grid, words, stq, 32, 1);
      return P;
    }
  }
  // Wide layers: K split four ways (lstm_bwd_persistent_ksplit_kernel) wherever the 16-sequence tile would be taken.  The caller
  // hands over the partial-sum exchange space the plan asks for (need_px): per (direction, 16-sequence tile) group and 64-unit block
  // 16 blocks of 16 x 16 words of 8 bytes (value, step), two slots by step parity (px_put / px_take), sized for the whole batch.
  if (bwd_ksplit_shape(L, stile)) {
    const int cpw = L.H / (32 * NW), gx = L.H / 64 * 4;
    const size_t px = (size_t)2 * L.ndir * cdiv(L.S, 16) * (size_t)(L.H / 64) * 4096 * 2;
    // Round 6: the same tile on two fp16 planes per operand (lstm_bwd_persistent_ksplit_h_kernel), for which the caller also hands over
    // the plane and exponent buffers (need_dgh, need_ex: 64 bytes per (t, dir, tile, producer)); batches that need two windows take
    // two launches of it (faster than one multiplexed fp32 launch)
    if (bwd_planes_shape(L, stile) && in_windows(rec_kernel(kBwdKsplitH, cpw), gx, 16, 64, 4)) {
      P.need_px = px; P.need_dgh = true;
      P.need_ex = (size_t)L.T * L.ndir * cdiv(L.S, 16) * (size_t)(L.H / 16) * 16;
      return P;
    }
    const RecKernel* k = rec_kernel(kBwdKsplit, cpw);
    const int nwin = !k ? 0 : pick_windows(L.S, 16, [&](int Sw) {
      const dim3 grid(gx, L.ndir, cdiv(Sw, 16));
      return ctl_words((size_t)grid.y * grid.z * 4) <= (size_t)kCtlHalf && fits(*k, grid);
    });
    // Two windows: one launch that time-multiplexes two sequence tiles per workgroup instead (lstm_bwd_persistent_ksplit_mux_kernel;
    // LstmLayerDev::bwd_mux = 0 / EESEN_BWD_MUX=0: the two launches, one after the other)
    if (nwin == 2 && L.bwd_mux && cpw >= 2 && cpw <= 4) {
      const int nz = cdiv(L.S, 16);
      const dim3 grid(gx, L.ndir, cdiv(nz, 2));
      const size_t words = ctl_words((size_t)L.ndir * nz * 4);   // one set per (direction, 16-sequence tile) and K quarter: every tile of the batch
      const RecKernel& km = *rec_kernel(kBwdKsplitMux, cpw);
      if (words <= (size_t)kCtlHalf && fits(km, grid)) {
        take(P, km, grid, words, 32, 64, 1);
        P.need_px = px;
        return P;
      }
    }
    if (nwin > 0 && (nwin == 1 || line_aligned(L.S / nwin, ldG))) {
      const dim3 grid(gx, L.ndir, cdiv(L.S / nwin, 16));
      take(P, *k, grid, ctl_words((size_t)grid.y * grid.z * 4), 16, 64, nwin);
      P.need_px = px;
      return P;
    }
  }
  in_windows(rec_kernel(kBwdGeneric, need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16, stile, L.drop_mode != 0), cdiv(L.H, 16), stile, 16, 1);
  return P;
}

void lstm_bwd_launch(hipStream_t st, const RecPlan& P, const LstmLayerDev& L0, const float* dY, int lddy, float* DG, unsigned* cnt,
                     unsigned* err, int spin_limit, unsigned long long* trace) {
  EESEN_REQUIRE(P.kind == kRecBwdQ4 || P.kind == kRecBwdKsplit || P.kind == kRecBwdKsplitMux || P.kind == kRecBwdGeneric, EESEN_ERR_STATE, "not a backward recurrence plan");
  EESEN_REQUIRE(!P.need_px || (L0.PX && L0.px_floats >= P.need_px), EESEN_ERR_STATE, "the backward plan's partial-sum exchange space (RecPlan::need_px) was not handed over");
  EESEN_REQUIRE(!P.need_dgh || (L0.DGH && L0.EX), EESEN_ERR_STATE, "the backward plan's plane and exponent buffers (RecPlan::need_dgh, need_ex) were not handed over");
  const RecRole role{P.grid[0], P.grid[1], P.grid[2], L0.xcd_map};
  const bool whole_batch = P.kind == kRecBwdQ4 || P.kind == kRecBwdKsplitMux;   // one launch: the kernel walks every sequence tile itself
  unsigned long long* px = reinterpret_cast<unsigned long long*>(L0.PX);
  int chunk = P.chunk;
  for (int w = 0; w < P.windows; ++w) {
    LstmLayerDev L = L0;
    if (whole_batch) { L.s_begin = 0; L.s_count = 0; }
    else { L.s_count = L0.S / P.windows; L.s_begin = w * L.s_count; }
    EESEN_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned) * P.ctl_words, st));
    if (P.need_px) EESEN_HIP_CHECK(hipMemsetAsync(L.PX, 0, sizeof(float) * P.need_px, st));
    if (P.kind == kRecBwdQ4) plan_launch(st, P.fn, P.wgs, L, dY, lddy, DG, cnt, err, spin_limit, trace, role);
    else if (P.kind == kRecBwdKsplitMux) plan_launch(st, P.fn, P.wgs, L, dY, lddy, DG, px, cnt, err, spin_limit, role, chunk);
    else if (P.kind == kRecBwdKsplit) plan_launch(st, P.fn, P.wgs, L, dY, lddy, DG, px, cnt, err, spin_limit, role, chunk, trace);
    else plan_launch(st, P.fn, P.wgs, L, dY, lddy, DG, cnt, err, spin_limit, trace, role, chunk);
  }
}

}  // namespace eesen
