// Which instantiation of which kernel family serves a problem of tangent dimension nv with md dense rows, and the one list
// of the instantiations that exist.  Plain C++: shared by the host side of the library (pinkhip.hip, launchers.h), by the
// one launcher translation unit (tu_kernel.hip), by the Makefile (which derives its objects from PINKHIP_FAMILIES with
// the preprocessor) and by the CPU wave emulator of the test suite, so that none of them can disagree about the rule.
#pragma once

// Every table has the shape X(NV, MD, W): NV = nv padded to the next instantiated even size (padded coordinates cost FMAs
// and LDS traffic), MD = dense rows the instantiation holds (0: the family takes md at run time or has none), W = lanes
// per QP (64 / W QPs per wavefront).  The order within a table is the rule "the smallest entry that holds it".
#ifdef PINKHIP_DEV_NV  // kernel-development builds: one instantiation only (make DEV=1 [DEVNV=50 DEVW=64 DEVMD=6], ~20 s)
#ifndef PINKHIP_DEV_MD
#define PINKHIP_DEV_MD 0
#endif
#if PINKHIP_DEV_NV > PINKHIP_DEV_W  // (front coordinates eliminated in the tableau kernel: the others hold all of them on 64 lanes)
#define PINKHIP_PACKED_TABLE(X) X(PINKHIP_DEV_NV, 0, 64)
#define PINKHIP_ROLLOUT_TABLE(X) X(PINKHIP_DEV_NV, 0, 64)
#else
#define PINKHIP_PACKED_TABLE(X) X(PINKHIP_DEV_NV, 0, PINKHIP_DEV_W)
#define PINKHIP_ROLLOUT_TABLE(X) X(PINKHIP_DEV_NV, 0, PINKHIP_DEV_W)
#endif
#if PINKHIP_DEV_MD > 0
#define PINKHIP_ROLLOUT_DENSE_TABLE(X) X(PINKHIP_DEV_NV, PINKHIP_DEV_MD, PINKHIP_DEV_W)
#else
#define PINKHIP_ROLLOUT_DENSE_TABLE(X)
#endif
#if PINKHIP_DEV_NV + PINKHIP_DEV_MD > PINKHIP_DEV_W  // (more tableau rows than lanes: the dense rows are virtual / front coordinates eliminated)
#define PINKHIP_SWEEP_TABLE(X) X(PINKHIP_DEV_NV, 0, PINKHIP_DEV_W)
#else
#define PINKHIP_SWEEP_TABLE(X) X(PINKHIP_DEV_NV, PINKHIP_DEV_MD, PINKHIP_DEV_W)
#endif
#if PINKHIP_DEV_MD > 0
#define PINKHIP_SWEEPX_TABLE(X) X(PINKHIP_DEV_NV, PINKHIP_DEV_MD, PINKHIP_DEV_W)
#define PINKHIP_WSWEEP_TABLE(X)
#define PINKHIP_WROLLOUT_TABLE(X)
#else
#define PINKHIP_SWEEPX_TABLE(X)
// (the warm-start twins of the one box-only instantiation)
#define PINKHIP_WSWEEP_TABLE(X) X(PINKHIP_DEV_NV, 0, PINKHIP_DEV_W)
#define PINKHIP_WROLLOUT_TABLE(X) PINKHIP_ROLLOUT_TABLE(X)
#endif
#define PINKHIP_RPAIRS_TABLE(X)  // (the sphere-pair kernels are not part of a development build)
#else
// the sweep-tableau kernel with VIRTUAL dense rows ik_solve_sweepx_kernel<NV, MD, W> (ik_sweepx.h): NV coordinates on the
// W lanes, up to MD dense rows riding in a second role of the first MD lanes (NV + MD may exceed W)
#define PINKHIP_SWEEPX_TABLE(X) X(16, 8, 16) X(30, 6, 32) X(30, 8, 32) X(32, 8, 32)
// the sweep-tableau kernel ik_solve_sweep_kernel<NV, MD, W> (ik_sweep.h): NV coordinates + MD dense rows
// = NT <= W tableau rows, one per lane -- or, box-only with NV > W: the first NV - W coordinates are eliminated before the
// solve (coordinates without bounds in every instance, pinkhip_desc::n_free_lead: the root of a free-flyer) and the other W
// ride on the lanes: X(34, 0, 32) = nv 33 / 34 two QPs per wavefront.  Ordered by NT within box-only / with dense rows; problems that fit none
// (8-lane groups, more dense rows than lanes are left) run the Goldfarb-Idnani kernel of PINKHIP_PACKED_TABLE.
#define PINKHIP_SWEEP_TABLE(X)                                                                                      \
  X(8, 0, 16) X(12, 0, 16) X(16, 0, 16) X(24, 0, 32) X(30, 0, 32) X(32, 0, 32) X(34, 0, 32) X(34, 0, 64) X(40, 0, 64) X(48, 0, 64) X(50, 0, 64) \
  X(56, 0, 64) X(64, 0, 64)                                                                                         \
  X(12, 4, 16) X(24, 8, 32) X(30, 2, 32) X(30, 8, 64) X(34, 8, 64) X(40, 8, 64) X(50, 6, 64) X(50, 14, 64) X(56, 8, 64)
// the whole-control-step kernel exists for the groups of whole 16-lane rows (broadcast-FMA stacking), box limits only
#define PINKHIP_ROLLOUT_TABLE(X) \
  X(12, 0, 16) X(16, 0, 16) X(24, 0, 32) X(30, 0, 32) X(32, 0, 32) X(34, 0, 64) X(40, 0, 64) X(48, 0, 64) X(50, 0, 64) X(56, 0, 64)
// ... and, with position-barrier rows formed on chip (NV + MD tableau rows on W lanes), for these
// (NV + MD > W: virtual dense rows, ik_sweepx.h; listed ahead of the wider group that would also hold the robot)
#define PINKHIP_ROLLOUT_DENSE_TABLE(X) X(12, 4, 16) X(30, 6, 32) X(30, 8, 64) X(34, 8, 64) X(50, 6, 64) X(50, 14, 64) X(56, 8, 64)
// Warm-start twins (box-only, started from the caller's active set: ik_sweep.h WARM) of the stack + solve kernel and of the
// whole-step kernel.  Sparse on purpose -- every entry is a translation unit of minutes: a shape runs on the smallest
// entry that holds it.
#define PINKHIP_WSWEEP_TABLE(X) X(16, 0, 16) X(30, 0, 32) X(34, 0, 32) X(50, 0, 64) X(64, 0, 64)
#define PINKHIP_WROLLOUT_TABLE(X) X(16, 0, 16) X(30, 0, 32) X(50, 0, 64) X(56, 0, 64)
// The whole-step kernel whose LAST dense rows are SelfCollisionBarrier rows of sphere pairs, selected and formed on chip
// (ik_rollout.h PAIRS).  Sparse like the warm-start twins: one row per lane at W = 16, virtual dense rows at W = 32, one
// robot per wavefront.
#define PINKHIP_RPAIRS_TABLE(X) X(12, 4, 16) X(30, 6, 32) X(50, 14, 64)
// the Goldfarb-Idnani kernel (ik_kernels_packed.h): dense rows are counted at run time, up to W of them
#define PINKHIP_PACKED_TABLE(X)                                                                      \
  X(6, 0, 8) X(8, 0, 8) X(12, 0, 16) X(16, 0, 16) X(24, 0, 32) X(30, 0, 32) X(32, 0, 32) X(34, 0, 64) X(40, 0, 64) X(48, 0, 64) X(50, 0, 64) \
  X(56, 0, 64) X(64, 0, 64)
#endif

// THE list of kernel families: F(KIND, DENSE, PREFIX, ARGS, TABLE) -- the PlanKind that launches it (+ LaunchPlan::dense:
// the packed kernel is built with and without the dense-row machinery), the prefix of its objects <PREFIX>_<NV>_<MD>_<W>.o,
// its argument struct and its table.  The launcher tables (launchers.h), the objects of the library (Makefile), has_entry()
// below and the emulator's registry (emu/emu_part.cpp) are generated from it.  A new family is one line here and one
// specialisation of pinkhip::Family next to its kernel.  Largest builds first: `make -j` starts objects in this order.
#define PINKHIP_FAMILIES(F)                                                         \
  F(PLAN_ROLLOUT_DENSE, 0, rdense, RolloutArgs, PINKHIP_ROLLOUT_DENSE_TABLE)        \
  F(PLAN_ROLLOUT_PAIRS, 0, rpairs, RolloutPairsArgs, PINKHIP_RPAIRS_TABLE)          \
  F(PLAN_ROLLOUT, 0, rollout, RolloutArgs, PINKHIP_ROLLOUT_TABLE)                   \
  F(PLAN_ROLLOUT_WARM, 0, wrollout, RolloutArgs, PINKHIP_WROLLOUT_TABLE)            \
  F(PLAN_SWEEPX, 0, sweepx, KernelArgs, PINKHIP_SWEEPX_TABLE)                       \
  F(PLAN_SWEEP, 0, sweep, KernelArgs, PINKHIP_SWEEP_TABLE)                          \
  F(PLAN_SWEEP_WARM, 0, wsweep, KernelArgs, PINKHIP_WSWEEP_TABLE)                   \
  F(PLAN_PACKED, 0, packed, KernelArgs, PINKHIP_PACKED_TABLE)                       \
  F(PLAN_PACKED, 1, pdense, KernelArgs, PINKHIP_PACKED_TABLE)

namespace pinkhip {

// What a launch plan (host_plan.h) launches
enum PlanKind {
  PLAN_NONE = 0,  // nothing to launch (B == 0)
  PLAN_STACK_SMALL,  // ik_stack_small_kernel<TP>: NV = 8, 64 / W instances per wavefront (W = 32: TP = 1, W = 8: TP = 4)
  PLAN_STACK_MFMA,   // ik_stack_mfma_kernel<NV / 16> (or its staged variant), W = 64
  PLAN_SWEEP,        // entry {NV, MD, W} of PINKHIP_SWEEP_TABLE
  PLAN_SWEEPX,       // ... of PINKHIP_SWEEPX_TABLE
  PLAN_PACKED,       // ... of PINKHIP_PACKED_TABLE, `dense`: the instantiation with the dense-row machinery
  PLAN_SWEEP_WARM,   // ... of PINKHIP_WSWEEP_TABLE
  PLAN_ROLLOUT,        // ... of PINKHIP_ROLLOUT_TABLE
  PLAN_ROLLOUT_DENSE,  // ... of PINKHIP_ROLLOUT_DENSE_TABLE
  PLAN_ROLLOUT_WARM,   // ... of PINKHIP_WROLLOUT_TABLE
  PLAN_ROLLOUT_PAIRS,  // ... of PINKHIP_RPAIRS_TABLE
};

// One launch: `blocks` wavefronts of 64 / W instances each
struct LaunchPlan {
  int kind, NV, MD, W, dense;
  long long blocks;
};

inline LaunchPlan make_plan(int kind, int NV, int MD, int W, int dense, long long B) {
  return LaunchPlan{kind, NV, MD, W, dense, (B + 64 / W - 1) / (64 / W)};
}

// What the one launcher (tu_kernel.hip) and the emulator's lane entries need to know about the family of `KIND`: its
// specialisations sit next to the kernels they describe (ik_kernels_packed.h, ik_sweep.h, ik_sweepx.h, ik_rollout.h) with
//   Args                 the argument struct
//   kernel               the __global__ instantiation
//   prepared(a)          the arguments as the kernel wants them (the tableau kernels: lds_pitch filled in)
//   lds_bytes(a), B(a)   dynamic LDS of a wavefront of 64 / W instances, batch size -- of prepared arguments
// and the static_asserts that tie the instantiation to what this file restates.
template <int KIND, int NV, int MD, int W, bool DENSE = false>
struct Family;

// Is {NV, MD, W} an entry of the table that plans of `kind` are launched from?
inline bool has_entry(int kind, int NV, int MD, int W) {
#define PINKHIP_ROW(NV_, MD_, W_) \
  if (NV == NV_ && MD == MD_ && W == W_) return true;
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) \
  if (kind == KIND) { TABLE(PINKHIP_ROW) }
  PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
#undef PINKHIP_ROW
  return false;
}

struct PackedChoice {
  int NV, W;
};

// Smallest instantiation that holds the problem.  Lane li < md of a group owns dense row li, so a group of W
// lanes takes at most W dense rows: up to PINKHIP_MAX_MD = 64 in the 64-lane instantiations (more rows than the
// smallest group for nv has lanes move the problem to a wider group).
inline PackedChoice select_packed(int nv, int md) {
#define PINKHIP_PICK(NV_, MD_, W_) \
  if (nv <= NV_ && md <= W_) return PackedChoice{NV_, W_};
  PINKHIP_PACKED_TABLE(PINKHIP_PICK)
#undef PINKHIP_PICK
  return PackedChoice{0, 0};
}

struct SweepChoice {
  int NV, MD, W;
};

// Smallest sweep-tableau instantiation that holds nv coordinates and md dense rows ({0, 0, 0}: none).
// n_free_lead: how many leading coordinates carry no bound in any instance (an instantiation that eliminates NV - W front
// coordinates needs that many)
inline SweepChoice select_sweep(int nv, int md, int n_free_lead = 0) {
#define PINKHIP_PICK(NV_, MD_, W_) \
  if (nv <= NV_ && md <= MD_ && (md > 0) == (MD_ > 0) && (NV_ <= W_ || n_free_lead >= NV_ - W_)) return SweepChoice{NV_, MD_, W_};
  PINKHIP_SWEEP_TABLE(PINKHIP_PICK)
#undef PINKHIP_PICK
  return SweepChoice{0, 0, 0};
}

// Smallest warm-start instantiation of the stack + solve kernel that holds nv coordinates ({0, 0, 0}: none; box-only)
inline SweepChoice select_sweep_warm(int nv, int n_free_lead = 0) {
#define PINKHIP_PICK(NV_, MD_, W_) \
  if (nv <= NV_ && (NV_ <= W_ || n_free_lead >= NV_ - W_)) return SweepChoice{NV_, MD_, W_};
  PINKHIP_WSWEEP_TABLE(PINKHIP_PICK)
#undef PINKHIP_PICK
  return SweepChoice{0, 0, 0};
}

// Smallest instantiation with virtual dense rows that holds nv coordinates and md > 0 dense rows ({0, 0, 0}: none).
inline SweepChoice select_sweepx(int nv, int md) {
  if (md <= 0) return SweepChoice{0, 0, 0};
#define PINKHIP_PICK(NV_, MD_, W_) \
  if (nv <= NV_ && md <= MD_) return SweepChoice{NV_, MD_, W_};
  PINKHIP_SWEEPX_TABLE(PINKHIP_PICK)
#undef PINKHIP_PICK
  return SweepChoice{0, 0, 0};
}

// ... and whether it is the kernel to run: when it packs more QPs into a wavefront than the instantiation with one
// lane per tableau row (nv = 30 with three to eight dense rows: two QPs per wavefront against one) -- or that one
// does not exist.
inline bool prefer_sweepx(int nv, int md) {
  const SweepChoice x = select_sweepx(nv, md);
  if (!x.NV) return false;
  const SweepChoice s = select_sweep(nv, md);
  return !s.NV || x.W < s.W;
}

// Which of the two stack + solve kernels serves a batch of B problems (measured on MI355X, scripts/ab_solvers.sh):
// the sweep-tableau kernel wherever it is instantiated, except
//   * when it needs a wider group than the Goldfarb-Idnani kernel (nv = 30 with six dense rows: 36 tableau rows = one QP
//     per wavefront against two: 1.75 against 1.46 ms per 65 536), and
//   * for nv <= 8 in large batches: its smallest group is 16 lanes, the Goldfarb-Idnani kernel packs eight QPs per
//     wavefront (UR5: 71 against 49 us at B = 65 536, but 13.8 against 18.4 us at B = 4 096, where eight per wavefront
//     leave half of the 1 024 SIMDs without a wave).
inline bool prefer_sweep(int nv, int md, long long B, int n_free_lead = 0) {
  const SweepChoice sc = select_sweep(nv, md, n_free_lead);
  if (!sc.NV) return false;
  const PackedChoice pc = select_packed(nv, md);
  if (!pc.NV) return true;
  if (nv <= 8) return B <= 16384;
  return sc.W <= pc.W;
}

// Doubles of LDS per QP of the sweep-tableau kernel (= SweepLds<NV, MD, W>::stride, checked at compile time by
// Family<PLAN_SWEEP>): H packed, c, the columns of G.
constexpr int sweep_lds_doubles(int NV, int MD, int W) { return ((NV * (NV + 1) / 2 + 1) & ~1) + 2 * W + MD * (W + 2); }

// ... of the kernel with virtual dense rows (= SweepXLds<NV, MD, W>::stride, checked by Family<PLAN_SWEEPX>)
constexpr int sweepx_lds_doubles(int NV, int MD, int W) { return ((NV * (NV + 1) / 2 + 1) & ~1) + W + MD * (W + 2) + 2 * ((MD + 1) & ~1); }

// Doubles of LDS per QP of the Goldfarb-Idnani kernel (= LdsP<NV>::stride(md), checked at compile time by
// the whole-step families): the sweep-tableau kernels hand a group over to it when its result fails the certificate.
constexpr int packed_lds_doubles(int NV, int md) {
  return ((((NV * (NV + 3) / 2 + 1) & ~1) + 5 * NV + md * (NV + 1)) + 1) & ~1;
}
constexpr int max3(int a, int b, int c) { return (a > b ? a : b) > c ? (a > b ? a : b) : c; }

// World positions of the nf task frames, kept BEHIND the area the kinematics and the two solvers share: the rows of
// position barriers are formed from them while the Goldfarb-Idnani code (hand-over) is already writing its staged rows.
// ... and, for up to kRolloutMaxEqFrames equality constraints made of frame tasks, U / V of their frames and their six errors
// (24 doubles each): the Goldfarb-Idnani code forms those rows too while the shared area is being overwritten.
constexpr int kRolloutMaxEqFrames = 2;
// (sized by the constraints the call has: a barrier-only stack does not pay LDS for them)
constexpr int rollout_tail_doubles(int nf, int n_eqf) { return ((3 * nf + 1) & ~1) + 24 * n_eqf; }

// Doubles of LDS per robot of the whole-control-step kernel: its kinematics scratch (fk_doubles) shares the solve's
// LDS, whichever is larger (+ the frame positions behind it when dense rows are formed on chip).
constexpr int rollout_lds_doubles(int NV, int W, int fk_doubles, int MD = 0, int nf = 0, int n_eqf = 0) {
  return max3((fk_doubles + 1) & ~1, NV + MD > W ? sweepx_lds_doubles(NV, MD, W) : sweep_lds_doubles(NV, MD, W), packed_lds_doubles(NV, MD)) +
         (MD > 0 ? rollout_tail_doubles(nf, n_eqf) : 0);
}

// Sphere-pair rows (ik_rollout.h PAIRS): behind the frame positions and the constraint copies the tail keeps the world
// centres of the spheres (3 each), the distance of every pair and five doubles per selected pair (normal, right-hand
// side, the two sphere indices)
constexpr int kPairsMaxSpheres = 32, kPairsMaxPairs = 64;
constexpr int rollout_pairs_doubles(int n_spheres, int n_pairs, int n_rows) { return (3 * n_spheres + n_pairs + 5 * n_rows + 1) & ~1; }

// Instantiation of the whole-control-step kernel for a robot with nv tangent coordinates and nj joints whose
// kinematics scratch needs fk_doubles doubles of LDS: W lanes must hold a joint / a column each, and the 64 / W
// robots of a wavefront must fit the 64 KiB of LDS a workgroup may ask for.
constexpr bool rollout_lds_fits(int doubles, int W) { return 8 * doubles * (64 / W) + 16 <= 65536; }

// An X-macro table as data, for the selectors below
struct TableEntry {
  int NV, MD, W;
};
#define PINKHIP_ROW(NV_, MD_, W_) {NV_, MD_, W_},
constexpr TableEntry kRolloutTable[] = {PINKHIP_ROLLOUT_TABLE(PINKHIP_ROW){0, 0, 0}};
constexpr TableEntry kRolloutDenseTable[] = {PINKHIP_ROLLOUT_DENSE_TABLE(PINKHIP_ROW){0, 0, 0}};
constexpr TableEntry kRolloutWarmTable[] = {PINKHIP_WROLLOUT_TABLE(PINKHIP_ROW){0, 0, 0}};
constexpr TableEntry kRolloutPairsTable[] = {PINKHIP_RPAIRS_TABLE(PINKHIP_ROW){0, 0, 0}};
#undef PINKHIP_ROW

// The smallest entry of `table` (closed by {0, 0, 0}) that holds the robot and md dense rows and whose LDS (+ extra
// doubles per robot) fits; first_decides: the first entry that holds the robot is taken or nothing ({0, 0, 0}: none)
inline SweepChoice select_rollout_entry(const TableEntry *table, int nv, int nj, int fk_doubles, int md, int nf, int n_eqf, int extra_doubles,
                                        bool first_decides = false) {
  for (const TableEntry *e = table; e->NV; ++e)
    if (nv <= e->NV && md <= e->MD && nj <= e->W) {
      if (rollout_lds_fits(rollout_lds_doubles(e->NV, e->W, fk_doubles, e->MD, nf, n_eqf) + extra_doubles, e->W)) return SweepChoice{e->NV, e->MD, e->W};
      if (first_decides) break;
    }
  return SweepChoice{0, 0, 0};
}

// ... with md > 0 rows of position barriers: {NV, MD, W} from PINKHIP_ROLLOUT_DENSE_TABLE
inline SweepChoice select_rollout_dense(int nv, int nj, int fk_doubles, int md, int nf, int n_eqf) {
  return select_rollout_entry(kRolloutDenseTable, nv, nj, fk_doubles, md, nf, n_eqf, 0);
}

// ... whose last rows are sphere-pair rows: {NV, MD, W} from PINKHIP_RPAIRS_TABLE
inline SweepChoice select_rollout_pairs(int nv, int nj, int fk_doubles, int md, int nf, int n_eqf, int pairs_doubles) {
  return select_rollout_entry(kRolloutPairsTable, nv, nj, fk_doubles, md, nf, n_eqf, pairs_doubles);
}

// ... started from the caller's active set: the smallest entry of PINKHIP_WROLLOUT_TABLE that holds the robot and whose LDS
// fits (explicitly asked for: no robot is sent back to the two-launch step)
inline PackedChoice select_rollout_warm(int nv, int nj, int fk_doubles) {
  const SweepChoice c = select_rollout_entry(kRolloutWarmTable, nv, nj, fk_doubles, 0, 0, 0, 0);
  return PackedChoice{c.NV, c.W};
}

// ... box limits only, PINKHIP_ROLLOUT_TABLE: the first entry that holds the robot decides
inline PackedChoice select_rollout(int nv, int nj, int fk_doubles, bool needed = false) {
  // robots that fit an 8-lane group keep the two-launch step: padding them to 16 lanes halves the robots per
  // wavefront (measured, 6-dof arm: 0.107 ms in one kernel at NV = 12 against 0.068 ms in two launches at NV = 6) --
  // unless the task stack has rows only this kernel forms (`needed`: constant rows, extra identity tasks, relative slots)
  if (nv <= 8 && !needed) return PackedChoice{0, 0};
  const SweepChoice c = select_rollout_entry(kRolloutTable, nv, nj, fk_doubles, 0, 0, 0, 0, true);
  return PackedChoice{c.NV, c.W};
}

}  // namespace pinkhip
