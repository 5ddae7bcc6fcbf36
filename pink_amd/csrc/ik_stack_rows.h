// Stacking of the task rows into H = damping I + sum_t (W_t J_t)^T (W_t J_t) + mu_t I, c = sum_t gain_t J_t^T W_t^2 e_t
// (pink/tasks/task.py:145-167, pink/solve_ik.py:54-60) for the kernels whose groups are whole rows of 16 lanes: lane li
// of a group accumulates row li of H in registers, fed by the broadcast-FMA of wave.h -- no LDS, no cross-lane
// reduction.  Shared by the Goldfarb-Idnani kernel (ik_kernels_packed.h) and the sweep-tableau kernel (ik_sweep.h).
#pragma once

#include "ik_common.h"

namespace pinkhip {

// Where the per-instance terms come from.  HbmTerms (default): the packed streams J / e / lb / ub in HBM.  A policy
// with kOnTheFly = true (ik_rollout.h: the whole-control-step kernel) produces the task rows, errors and bounds
// itself -- frame_rows(f, dst) fills this lane's entries of the six rows of FrameTask f, error(k) / diag_error(r)
// return task errors, lb / ub are members -- and receives the result back in x / status.
struct HbmTerms {
  static constexpr bool kOnTheFly = false;
  double lb = 0.0, ub = 0.0, x = 0.0;
  int status = 0;
  __device__ __forceinline__ void frame_rows(int, double (&)[6]) const {}
  __device__ __forceinline__ double error(int) const { return 0.0; }
  __device__ __forceinline__ double diag_error(int) const { return 0.0; }
  __device__ __forceinline__ double dense_col(int) const { return 0.0; }
  __device__ __forceinline__ double dense_h(int) const { return 0.0; }
};

// Dense task rows.  Lane li requests J[k][li] for the RC rows of a chunk (one coalesced request per row), lane k the
// weights of row k; DEPTH chunks are in flight ahead of the one being accumulated.  Row k then enters every lane's H
// row through the broadcast-FMA:  H[li][j] += (w_k^2 J[k][li]) * J[k][j]  with J[k][j] taken from lane j and w_k^2
// from lane k.  M holds at least NV entries (the first NV are used); ci and mu_l accumulate this lane's entry of c
// and its share of the Levenberg-Marquardt term.
// DEPTH: a chunk of eight rows is accumulated in ~1 k cycles of this wave's own issue time, a request takes several
// thousand under load -- with ONE chunk ahead (DEPTH = 1) a lone wave waits out the memory latency once per chunk
// (section clock, round 4: 30 k cycles per wave in this phase, whatever the input regime); DEPTH = 2 has all 24 rows of
// the headline stack in flight before the first FMA.  The stack + solve kernels at three waves per SIMD are built with
// DEPTH = 1 (ik_sweep.h: PINKHIP_STACK_DEPTH -- the other waves of the SIMD issue during the wait, and the third chunk
// buffer is 20 registers the kernel does not have), those at two waves per SIMD with DEPTH = 2
// (PINKHIP_STACK_DEPTH_WIDE).  (an on-the-fly source delivers one FrameTask = six rows per chunk and nothing is in flight)
// `mid` runs between the first requests and the first accumulation: what else the caller wants from HBM (bounds,
// the terms of the diagonal tasks) is requested there and arrives within the same wait.
struct NoMid {
  __device__ __forceinline__ void operator()() const {}
};
// NX > 0: the task rows have NX columns IN FRONT of the ones the lanes hold (a.J points at column NX of row 0; ik_sweep.h:
// coordinates that are eliminated before the solve).  Their entries are group-uniform: lane kk of a chunk requests
// J[r0 + kk][x - NX] with its weights and the rows hand them round with the broadcast that hands the weights round.
// Collected: this lane's entries H[li][x] in m[x], and PER-LANE PARTIAL sums of the uniform entries (to be summed over
// the group by the caller): hxx[0] = H[0][0], and for NX = 2 hxx[1] = H[0][1], hxx[2] = H[1][1]; cx[x] = c[x].
template <int NX>
struct StackFront {
  double m[NX > 0 ? NX : 1] = {};
  double hxx[NX > 0 ? NX * (NX + 1) / 2 : 1] = {};
  double cx[NX > 0 ? NX : 1] = {};
};
// Where the instances of a wave sit in the batch (SPLIT below): the first one, `first` -- the same in every lane, so that
// whatever is formed from it and from kernel arguments is scalar arithmetic on a scalar pointer -- and this lane's
// instance counted from it, `rel` (0 .. 64 / W - 1).  A lane's entry of a [B, pitch] stream is then
// (stream + first * pitch)[rel * pitch + li]: a scalar base and ONE 32-bit offset per lane, whatever the pitch, in the
// place of a 64-bit product and sum per lane and request.
struct WaveSplit {
  long long first = 0;
  unsigned rel = 0;
};
// ... for the sources that read their terms from HBM.  The whole-step kernel reads next to nothing per instance here (its
// rows are formed on chip) and holds the state of its kinematics in scalar registers at this point: the scalar bases were
// registers it did not have (spilled SGPRs in most of its instantiations), so it keeps the per-lane addresses.
#ifndef PINKHIP_WAVE_SPLIT
#define PINKHIP_WAVE_SPLIT(Src) (!Src::kOnTheFly)
#endif
// Three switches of the stacking that remove work and change no bit of any result, on where the streams are addressed through
// a WaveSplit (DIAG below: the stack + solve kernels with rows from HBM); off, the device code is what it was.
//   ROLE_BUFFERS     the chunk loop is unrolled by the number of chunk buffers, so that a buffer changes its ROLE from trip to
//                    trip -- requested into, accumulated from -- instead of being copied into its neighbour at the end of
//                    every chunk (Kd is a run-time value, the loop is rolled: `buf[d] = buf[d + 1]` was 12 v_mov_b64 per
//                    chunk of eight rows at DEPTH = 1).  The same requests, the same rows in the same order.
//   SKIP_ZERO_ROWS   a task row whose weight is exactly zero is not multiplied (a FrameTask with orientation cost 0, as in
//                    examples/humanoid_draco3.py; the slots of frames that only a barrier needs).  One ballot
//                    per chunk over `wa == 0 && gw == 0` in the lane that holds the row's weights; row kk is a CANDIDATE if
//                    that holds in lane kk of EVERY group of the wave (per-instance costs: in both instances); a candidate
//                    is skipped if one more ballot finds every lane's entry of the row finite, and with NX > 0 the row's front
//                    entries (lane kk's px) finite as well.  Every other row takes the ordinary path.  Why no bit changes:
//                      * what the row would add to an accumulator is (+-0 * finite) or (finite * +-0): +-0 -- aa itself
//                        is fma(+-0, r, +0) = +0 for a finite r, the products into M[j], *hdiag and front->m are +-0 * finite,
//                        the one into ci is (gw = +-0) * finite;
//                      * every one of those accumulators starts at +0.0 and only ever receives sums under
//                        round-to-nearest, which give -0.0 only for (-0) + (-0) -- and, the one exception, for an FMA
//                        whose exact result is negative and below half the smallest denormal (|product| < 2^-1075 into an
//                        accumulator that is still zero): that rounds to -0.0.  Short of that underflow none of them is
//                        ever -0.0;
//                      * so acc + (+-0) == acc bit for bit, zero or not.  (In the underflow case the multiplied row
//                        would turn the -0.0 into +0.0 and the skipped one leaves it: a zero of the other sign, with
//                        entries of J below 1e-160.)
//                    A NaN gw (a non-finite error or gain: 0 * inf, 0 * NaN) fails the first compare, an inf or NaN in the
//                    row the second: the NaN such a row makes of H is made as before.  The per-lane terms outside the row
//                    loop (mu_l, the front's hxx / cx) are computed as before.  The row is still requested: the finite test
//                    needs it, and the kernel is not short of HBM bandwidth.
#ifndef PINKHIP_STACK_ROLE_BUFFERS
#define PINKHIP_STACK_ROLE_BUFFERS(Src) PINKHIP_WAVE_SPLIT(Src)
#endif
#ifndef PINKHIP_STACK_SKIP_ZERO_ROWS
#define PINKHIP_STACK_SKIP_ZERO_ROWS(Src) PINKHIP_WAVE_SPLIT(Src)
#endif
//   FULL_CHUNKS      a chunk that is full (Kd - r0 >= RC, wave-uniform: every chunk of the headline's 24 rows) is requested
//                    without the per-row `kk < rc`: ONE region of the lanes `in` around its RC row loads, the row's address a
//                    scalar pointer that advances by the run-time pitch (nv doubles) from row to row -- no (r0 + kk) * nv per
//                    row -- and this lane's part the 32-bit BYTE offset 8 voJ, so that the load takes the scalar base and
//                    the 32-bit offset as they are (global_load_dwordx2 v, v, s[:]) instead of a 64-bit sum per lane and
//                    row.  The same loads from the same addresses (8 voJ < 2^32: the instances of a wave hold less than
//                    4 GiB of task rows -- host_plan.h: rows_within_lane_offset sends anything else to another kernel); the
//                    lanes li >= nv get their zeros as before.  A partial chunk -- the last one of a Kd that is no multiple
//                    of RC -- makes the requests it always made, inside the same region: `kk < rc` is a scalar branch there.
//                    The weights, errors, gains, LM factors and front columns are requested as they were, by the lanes
//                    li < rc: on a full chunk that guard is one s_min and one v_cmp, and a second copy of those requests for
//                    `li < RC` would stand next to the first as the two forms of the row requests first did (request()).
//                    Needs ROLE_BUFFERS (the buffers keep their registers).
#ifndef PINKHIP_STACK_FULL_CHUNKS
#define PINKHIP_STACK_FULL_CHUNKS(Src) PINKHIP_WAVE_SPLIT(Src)
#endif
// DIAG: *hdiag follows this lane's own diagonal entry M[li] (lane li, li < NV) in a register of its own -- the product the
// broadcast-FMA of column li forms in lane li is this lane's own row entry times its own factor: the same FMA on the
// same operands, bit for bit what M[li] receives -- so that the caller does not have to pick "register li of lane li"
// out of the row afterwards (NV compares and 2 NV selects).  It also takes the instance as `ws` (b = ws.first + ws.rel)
// and addresses the streams as described at WaveSplit: the same addresses.  Off: nothing changes.
// ROLE_OK, FULL_OK: the caller's veto of ROLE_BUFFERS / FULL_CHUNKS for an instantiation in which the unrolled loop / the second
// form of the requests costs registers.
template <int NV, int W, int RCMAX, class Src, int DEPTH = 1, int NX = 0, bool DIAG = false, bool ROLE_OK = true, bool FULL_OK = true, int NM,
          class Mid = NoMid>
__device__ __forceinline__ void stack_rows_bcast(const KernelArgs &a, long long b, Src *terms, bool in, int li,
                                                 double (&M)[NM], double &ci, double &mu_l, Mid mid = Mid(), StackFront<NX> *front = nullptr,
                                                 double *hdiag = nullptr, WaveSplit ws = WaveSplit()) {
  static_assert(NX >= 0 && NX <= 2 && (NX == 0 || !Src::kOnTheFly), "at most two front columns, from HBM");
  static_assert(NM >= NV && W >= 16, "row-group kernels only");
  using BcT = Bcast<W>;
  const int nv = a.nv, Kd = a.Kd, K = a.K;
  // (SPLIT: the scalar bases of the wave and this lane's offsets from them; a.cost is per instance or one for all)
  constexpr bool SPLIT = DIAG && PINKHIP_WAVE_SPLIT(Src);
  constexpr bool ROLES = SPLIT && ROLE_OK && PINKHIP_STACK_ROLE_BUFFERS(Src);
  constexpr bool ZSKIP = SPLIT && PINKHIP_STACK_SKIP_ZERO_ROWS(Src);
  constexpr bool FULL = ROLES && FULL_OK && !Src::kOnTheFly && PINKHIP_STACK_FULL_CHUNKS(Src);  // (the buffers keep their registers)
  const double *Jb = a.J + (SPLIT ? ws.first : b) * (long long)Kd * nv;
  const double *eb = a.e + (SPLIT ? ws.first : b) * (long long)K;
  const double *costb = a.cost_batched ? a.cost + (SPLIT ? ws.first : b) * (long long)K : a.cost;
  const unsigned voJ = SPLIT ? ws.rel * static_cast<unsigned>(Kd * nv) + li : 0u;
  const unsigned voJ8 = voJ * 8u;  // (FULL: in bytes)
  const unsigned voE = SPLIT ? ws.rel * static_cast<unsigned>(K) + li : 0u;
  const unsigned voC = (SPLIT && a.cost_batched) ? voE : static_cast<unsigned>(li);
  constexpr int RC = Src::kOnTheFly ? 6 : (RCMAX < 8 ? RCMAX : 8);
  constexpr int NB = Src::kOnTheFly ? 2 : DEPTH + 1;  // chunk buffers: the one being accumulated + those in flight
  static_assert(RC <= 16, "weight rows are broadcast from the first row of 16 lanes");
  struct Chunk {
    double r[RC];
    double pw, pe, pg, pl;
    double px[NX > 0 ? NX : 1];
  };
  Chunk buf[NB];
  // (hold: the request is made inside the chunk loop -- FULL: this lane's offset is pinned there, wave.h: opaque_offset)
  auto request = [&](Chunk &dst, int r0, bool hold = false) {
    const int rc = (Kd - r0 < RC) ? Kd - r0 : RC;  // (<= 0: past the end, nothing is read)
    if constexpr (Src::kOnTheFly) {
      double six[6];
      terms->frame_rows(r0 / 6, six);
#pragma unroll
      for (int kk = 0; kk < RC; ++kk) dst.r[kk] = (in && kk < rc) ? six[kk] : 0.0;
    } else if constexpr (FULL) {
      // The defaults first, for every lane; then ONE region of the lanes `in`, and inside it nothing but wave-uniform
      // branches: the full chunk's RC loads from a scalar row pointer, or the rows kk < rc of a partial one.  (The two
      // forms side by side, each with its own region of lanes and its own defaults, are linearised one behind the other, and
      // the defaults of the second then follow, as far as the wait counters can tell, the loads of the first into the same
      // registers: every request waited for everything in flight.)
#pragma unroll
      for (int kk = 0; kk < RC; ++kk) dst.r[kk] = 0.0;
      if (in) {
        if (Kd - r0 >= RC) {  // a full chunk
          const char *row = reinterpret_cast<const char *>(Jb + (long long)r0 * nv);  // (scalar)
          const long long pitch = (long long)nv * 8;
          // (pinned in the loop only: in front of it the offset is formed next to the load anyway, and a volatile asm ahead of
          // `mid` would cost its table reads their scalar loads)
          const unsigned vo8 = hold ? opaque_offset(voJ8) : voJ8;
#pragma unroll
          for (int kk = 0; kk < RC; ++kk) {
            dst.r[kk] = *reinterpret_cast<const double *>(row + vo8);
            row += pitch;
          }
        } else {
#pragma unroll
          for (int kk = 0; kk < RC; ++kk)
            if (kk < rc) dst.r[kk] = (Jb + (long long)(r0 + kk) * nv)[voJ];
        }
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < RC; ++kk) {
        if constexpr (SPLIT) dst.r[kk] = (in && kk < rc) ? (Jb + (long long)(r0 + kk) * nv)[voJ] : 0.0;
        else dst.r[kk] = (in && kk < rc) ? Jb[(long long)(r0 + kk) * nv + li] : 0.0;
      }
    }
    dst.pw = dst.pe = dst.pg = dst.pl = 0.0;
    if constexpr (NX > 0) {
#pragma unroll
      for (int x = 0; x < NX; ++x) {
        if constexpr (SPLIT) dst.px[x] = (li < rc) ? (Jb + ((long long)r0 * nv - NX + x))[voJ - li + static_cast<unsigned>(li * nv)] : 0.0;
        else dst.px[x] = (li < rc) ? Jb[(long long)(r0 + li) * nv - NX + x] : 0.0;
      }
    }
    if (li < rc) {
      const int k = r0 + li;
      if constexpr (SPLIT) {
        dst.pw = (costb + r0)[voC];
        if constexpr (Src::kOnTheFly) dst.pe = terms->error(k);
        else dst.pe = (eb + r0)[voE];
        dst.pg = (a.row_gain + r0)[static_cast<unsigned>(li)];
        dst.pl = (a.row_lm + r0)[static_cast<unsigned>(li)];
      } else {
        dst.pw = costb[k];
        if constexpr (Src::kOnTheFly) dst.pe = terms->error(k);
        else dst.pe = eb[k];
        dst.pg = a.row_gain[k];
        dst.pl = a.row_lm[k];
      }
    }
  };
  auto forget_chunk = [&](Chunk &dst) {
#pragma unroll
    for (int kk = 0; kk < RC; ++kk) forget(dst.r[kk]);
    forget(dst.pw), forget(dst.pe), forget(dst.pg), forget(dst.pl);
#pragma unroll
    for (int x = 0; x < NX; ++x) forget(dst.px[x]);
  };
  if (Kd > 0) {
#pragma unroll
    for (int d = 0; d < NB - 1; ++d)
      if (d * RC < Kd) request(buf[d], d * RC);  // wave-uniform
  }
  mid();
  if constexpr (!ROLES && !ZSKIP) {
    // (the switches off: this loop as it always was -- the device code of its users does not change by a byte)
    for (int r0 = 0; r0 < Kd; r0 += RC) {
      const int rc = (Kd - r0 < RC) ? Kd - r0 : RC;
      if (r0 + (NB - 1) * RC < Kd) request(buf[NB - 1], r0 + (NB - 1) * RC);
      const Chunk &cur = buf[0];
      const double wa = (li < rc) ? cur.pw * cur.pw : 0.0;
      const double gw = (li < rc) ? cur.pg * wa * cur.pe : 0.0;
      if (li < rc) mu_l += cur.pl * (cur.pg * cur.pg) * wa * cur.pe * cur.pe;
      const BcT wab = bcast_prepare<W>(wa), gwb = bcast_prepare<W>(gw);
      BcT pxb[NX > 0 ? NX : 1];
      if constexpr (NX > 0) {
        // (lane kk's own row: its part of the uniform entries)
        front->hxx[0] = fma(wa * cur.px[0], cur.px[0], front->hxx[0]);
        front->cx[0] = fma(gw, cur.px[0], front->cx[0]);
        if constexpr (NX == 2) {
          front->hxx[1] = fma(wa * cur.px[0], cur.px[1], front->hxx[1]);
          front->hxx[2] = fma(wa * cur.px[1], cur.px[1], front->hxx[2]);
          front->cx[1] = fma(gw, cur.px[1], front->cx[1]);
        }
#pragma unroll
        for (int x = 0; x < NX; ++x) pxb[x] = bcast_prepare<W>(cur.px[x]);
      }
      static_for<0, RC>([&](auto Kc) {
        constexpr int kk = decltype(Kc)::value;
        if (kk < rc) {  // wave-uniform
          // (the row's own uses first: the row copies of the broadcast are then made in its registers)
          const double aa = fma_bcast<W, kk>(0.0, wab, cur.r[kk]);
          ci = fma_bcast<W, kk>(ci, gwb, cur.r[kk]);
          if constexpr (DIAG) *hdiag = fma(cur.r[kk], aa, *hdiag);
          const BcT rowb = bcast_prepare<W>(cur.r[kk]);
          static_for<0, NV>([&](auto Jc) {
            constexpr int j = decltype(Jc)::value;
            M[j] = fma_bcast<W, j>(M[j], rowb, aa);
          });
          if constexpr (NX > 0) {
#pragma unroll
            for (int x = 0; x < NX; ++x) front->m[x] = fma_bcast<W, kk>(front->m[x], pxb[x], aa);  // H[li][x] += (w^2 J[k][li]) J[k][x]
          }
        }
      });
#pragma unroll
      for (int d = 0; d + 1 < NB; ++d) buf[d] = buf[d + 1];
    }
  } else {
    // chunk [r0, r0 + RC) out of `cur`
    auto accumulate = [&](const Chunk &cur, int r0) {
      const int rc = (Kd - r0 < RC) ? Kd - r0 : RC;
      const double wa = (li < rc) ? cur.pw * cur.pw : 0.0;
      const double gw = (li < rc) ? cur.pg * wa * cur.pe : 0.0;
      if (li < rc) mu_l += cur.pl * (cur.pg * cur.pg) * wa * cur.pe * cur.pe;
      // bit kk: row kk of the chunk is multiplied (wave-uniform, scalar)
      unsigned live = rc >= RC ? (1u << RC) - 1u : (1u << rc) - 1u;
      if constexpr (ZSKIP) {
        // (lanes li >= rc have wa = gw = 0: their bits are set, and `live` has none for them)
        unsigned long long cand = wave_ballot(wa == 0.0 && gw == 0.0);
#pragma unroll
        for (int g = 1; g < kWave / W; ++g) cand &= cand >> (W & 63);  // (bit kk < W: lane kk of every group)
        unsigned c = static_cast<unsigned>(cand) & live;
        // wave-uniform: no chunk of a stack without zero weights comes here (the test is on a copy the compiler cannot see
        // through: it would replace this one branch by the RC tests of the single bits)
        if (opaque_uniform(static_cast<int>(c)) != 0) {
          if constexpr (NX > 0) {
            bool pf = fabs(cur.px[0]) < INFINITY;  // (false for an inf and for a NaN)
            if constexpr (NX == 2) pf = pf && fabs(cur.px[1]) < INFINITY;
            unsigned long long pm = wave_ballot(pf);
#pragma unroll
            for (int g = 1; g < kWave / W; ++g) pm &= pm >> (W & 63);
            c &= static_cast<unsigned>(pm);
          }
          static_for<0, RC>([&](auto Kc) {
            constexpr int kk = decltype(Kc)::value;
            if ((c >> kk) & 1u) {
              if (wave_ballot(!(fabs(cur.r[kk]) < INFINITY)) == 0ull) live &= ~(1u << kk);
            }
          });
        }
      }
      const BcT wab = bcast_prepare<W>(wa), gwb = bcast_prepare<W>(gw);
      BcT pxb[NX > 0 ? NX : 1];
      if constexpr (NX > 0) {
        // (lane kk's own row: its part of the uniform entries)
        front->hxx[0] = fma(wa * cur.px[0], cur.px[0], front->hxx[0]);
        front->cx[0] = fma(gw, cur.px[0], front->cx[0]);
        if constexpr (NX == 2) {
          front->hxx[1] = fma(wa * cur.px[0], cur.px[1], front->hxx[1]);
          front->hxx[2] = fma(wa * cur.px[1], cur.px[1], front->hxx[2]);
          front->cx[1] = fma(gw, cur.px[1], front->cx[1]);
        }
#pragma unroll
        for (int x = 0; x < NX; ++x) pxb[x] = bcast_prepare<W>(cur.px[x]);
      }
      static_for<0, RC>([&](auto Kc) {
        constexpr int kk = decltype(Kc)::value;
        if (ZSKIP ? __builtin_expect(((live >> kk) & 1u) != 0u, 1) : kk < rc) {  // wave-uniform
          // (the row's own uses first: the row copies of the broadcast are then made in its registers)
          const double aa = fma_bcast<W, kk>(0.0, wab, cur.r[kk]);
          ci = fma_bcast<W, kk>(ci, gwb, cur.r[kk]);
          if constexpr (DIAG) *hdiag = fma(cur.r[kk], aa, *hdiag);
          const BcT rowb = bcast_prepare<W>(cur.r[kk]);
          static_for<0, NV>([&](auto Jc) {
            constexpr int j = decltype(Jc)::value;
            M[j] = fma_bcast<W, j>(M[j], rowb, aa);
          });
          if constexpr (NX > 0) {
#pragma unroll
            for (int x = 0; x < NX; ++x) front->m[x] = fma_bcast<W, kk>(front->m[x], pxb[x], aa);  // H[li][x] += (w^2 J[k][li]) J[k][x]
          }
        }
      });
    };
    if constexpr (ROLES) {
      // NB chunks per trip: chunk s of a trip is accumulated out of buf[s] while buf[s - 1] -- free since the chunk before --
      // takes the request NB - 1 chunks ahead
      for (int r0 = 0; r0 < Kd; r0 += NB * RC) {
        static_for<0, NB>([&](auto Sc) {
          constexpr int s = decltype(Sc)::value;
          const int r = r0 + s * RC;
          if (r < Kd) {  // wave-uniform
            // (no request: the buffer's registers are dead, and said to be -- carried round the loop as they were, a row's
            // permlane swaps would have to spare them: two more v_mov_b32 per row)
            if (r + (NB - 1) * RC < Kd) request(buf[(s + NB - 1) % NB], r + (NB - 1) * RC, true);
            else forget_chunk(buf[(s + NB - 1) % NB]);
            accumulate(buf[s], r);
          } else {
            forget_chunk(buf[(s + NB - 1) % NB]);
          }
        });
      }
    } else {
      for (int r0 = 0; r0 < Kd; r0 += RC) {
        if (r0 + (NB - 1) * RC < Kd) request(buf[NB - 1], r0 + (NB - 1) * RC);
        accumulate(buf[0], r0);
#pragma unroll
        for (int d = 0; d + 1 < NB; ++d) buf[d] = buf[d + 1];
      }
    }
  }
}

// Diagonal tasks (J = eye[col0 : col0 + k], PostureTask posture_task.py:128-129, DampingTask ...): their Jacobian is
// never stored.  Returns what they add to this lane's diagonal entry; c and the LM term accumulate in ci / mu_l.
template <class Src>
__device__ __forceinline__ double stack_diag_tasks(const KernelArgs &a, long long b, Src *terms, int li, double &ci,
                                                   double &mu_l) {
  const double *eb = a.e + b * (long long)a.K;
  const double *costb = a.cost_batched ? a.cost + b * (long long)a.K : a.cost;
  double dadd = 0.0;
  for (int t = 0; t < a.n_dtasks; ++t) {
    const int off = li - a.dtask_col0[t];
    if (off >= 0 && off < a.dtask_k[t]) {
      const int r = a.dtask_row0[t] + off;
      const double w = costb[r], gn = a.row_gain[r], l = a.row_lm[r];
      double ev;
      if constexpr (Src::kOnTheFly) ev = terms->diag_error(r);
      else ev = eb[r];
      const double wa = w * w;
      dadd += wa;
      ci += gn * wa * ev;
      mu_l += l * (gn * gn) * wa * ev * ev;
    }
  }
  return dadd;
}

// ... with the instance as a WaveSplit: the same terms from the same addresses
template <class Src>
__device__ __forceinline__ double stack_diag_tasks(const KernelArgs &a, WaveSplit ws, Src *terms, int li, double &ci,
                                                   double &mu_l) {
  const double *eb = a.e + ws.first * (long long)a.K;
  const double *costb = a.cost_batched ? a.cost + ws.first * (long long)a.K : a.cost;
  const unsigned vo = ws.rel * static_cast<unsigned>(a.K);
  const unsigned voc = a.cost_batched ? vo : 0u;
  double dadd = 0.0;
  for (int t = 0; t < a.n_dtasks; ++t) {
    const int off = li - a.dtask_col0[t];
    if (off >= 0 && off < a.dtask_k[t]) {
      const int r = a.dtask_row0[t] + off;
      const double w = costb[voc + static_cast<unsigned>(r)], gn = a.row_gain[r], l = a.row_lm[r];
      double ev;
      if constexpr (Src::kOnTheFly) ev = terms->diag_error(r);
      else ev = eb[vo + static_cast<unsigned>(r)];
      const double wa = w * w;
      dadd += wa;
      ci += gn * wa * ev;
      mu_l += l * (gn * gn) * wa * ev * ev;
    }
  }
  return dadd;
}

}  // namespace pinkhip
