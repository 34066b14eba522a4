// tmx_check.h — batched trajectory collision check (tmx_check_trajectories / tmx_best_trajectories_checked).
//
// What the reference's tests do with tesseract's checkTrajectory(contacts, manager, state_solver, joint_names, traj, config)
// (trajopt/test/cast_cost_unit.cpp:83-117 and its twins): every contact (step t, sub-state or swept sub-segment i, link primitive s,
// obstacle o) of a trajectory at the resolution of a CollisionCheckConfig, on the geometry of this library.  The distances are the
// ones of the collision terms - contact_distance_at for the discrete types, the swept branch of lvs_contact for the cast types, the
// sub-state rule of lvs_contact (lin_spaced_at) - but nothing here knows about row slots: no safety_margin_buffer, no fixed_steps, no
// removeInvalidContactResults, steps 0 .. T-1.
//
// k_check_trajectories: workgroup (chunk c, trajectory b) owns the steps [c * spc, (c + 1) * spc) of trajectory b and walks them one
// after the other.  The items k = (i * S + s) * O + o of a step are processed in TILES of at most `tile` items, ascending:
//   phase 1  one thread per sub-state of the tile: interpolated joint values, ONE walk of the chain, the world frame of every link up
//            to the last one that carries a primitive goes to LDS (12 doubles per frame).  lvs_contact walks the chain for every
//            (slot, end state); here a sub-state is walked once for all S x O pairs and for both sub-segments that meet in it (the
//            end of sub-segment i IS the start of i + 1: the same LDS frame).
//   phase 2  the items strided over the threads: the geometry routine the term code selects, the distance to an LDS table.
//   phase 3  every thread scans one contiguous block of the table (minimum with its item, number of items below the margin); thread 0
//            then takes the blocks in ascending order: the minimum (strict <: the lowest item wins a tie) and the hinge sum, which
//            it adds item by item in ascending order - only in blocks that hold an item below the margin (x + 0.0 == x for the
//            others).  The running (minimum, item, sum) of thread 0 is carried from tile to tile.
// So every result is the left fold over the ascending items whatever the number of threads, chunks or tiles: the host build (one
// thread), the SIMT emulation and the device give the same bytes.  No atomics, no hand-off between workgroups.
// The HULL twin carries GJK / EPA (include/tmx_gjk.h) and is launched only for problems with convex-hull links.
#pragma once
#include "tmx_terms.h"

struct CheckArgs
{
  int type;            // tmx_check_config::evaluator_type, 0 .. 4
  int kmax;            // cap of sub-states per segment (>= 2)
  int tile;            // items per tile (>= 1)
  int fcap;            // sub-state frames the LDS holds (>= tile / (S * O) + 3)
  int spc, chunks;     // steps per chunk, chunks per trajectory
  int converged_only;  // 1: trajectories whose status differs from converged_code are skipped (tmx_best_trajectories_checked)
  int converged_code;
  double margin, lvs;
};
// doubles of dynamic LDS: frames, distance table, block minima, and 2 ints per thread (block item, block count)
TMX_HOSTDEVFN size_t check_lds_doubles(int DK, int tile, int fcap, int NT)
{
  return (size_t)fcap * DK * 12 + (size_t)tile + (size_t)NT + (size_t)NT + 2;
}

// world frames of links 0 .. upto at the joint values qat(k): fk_link_visit's left-to-right product, the frame of link k is its value
// after joint k (what fk_link_at(P, qat, k, .) returns, operation by operation); out = 12 doubles per link (R row-major, then t)
template <class QAt>
TMX_DEVFN void check_link_frames(const DevProblem* P, QAt&& qat, int upto, double* out)
{
  Tf3 T, O, M, U;
  tf_from12(P->base, T);
  for (int k = 0; k <= upto; ++k)
  {
    tf_from12(P->origin[k], O);
    tf_mul(T, O, U);
    tf_joint_motion(P->axis[k], P->jtype[k], qat(k), M);
    tf_mul(U, M, T);
    for (int e = 0; e < 9; ++e)
      out[12 * k + e] = T.R[e];
    for (int e = 0; e < 3; ++e)
      out[12 * k + 9 + e] = T.t[e];
  }
}
TMX_DEVFN void check_load_frame(const double* f, Tf3& T)
{
  for (int e = 0; e < 9; ++e)
    T.R[e] = f[e];
  for (int e = 0; e < 3; ++e)
    T.t[e] = f[9 + e];
}

// signed distance of link primitive s, swept from placement Ta to placement Tb of its link, to obstacle o: the cast branch of
// lvs_contact (tmx_terms.h), selection by selection
template <bool HULL>
TMX_DEVFN double check_swept_distance(const DevProblem* P, const Tf3& Ta, const Tf3& Tb, int s, int o)
{
  double p[3], oq[3], n[3];
  int inside = 0;
  double tau = 0.0;
  bool hull = false;
  if constexpr (HULL)
    hull = P->n_ls_hull > 0 && P->ls_hull[2 * s + 1] > 0;
  if (hull)
  {
    inside = hull_closest_nl(P->hull + 3 * P->ls_hull[2 * s], P->ls_hull[2 * s + 1], Ta.R, Ta.t, Tb.R, Tb.t, P->ob_center + 3 * o, P->ob_axis + 3 * o,
                             P->n_ob_box > 0 ? P->ob_box + 12 * o : nullptr, P->mesh, p, oq, &tau);
  }
  else
  {
    double ca[3], cb[3];
    for (int rr = 0; rr < 3; ++rr)
    {
      ca[rr] = Ta.R[3 * rr + 0] * P->ls_center[3 * s + 0] + Ta.R[3 * rr + 1] * P->ls_center[3 * s + 1] + Ta.R[3 * rr + 2] * P->ls_center[3 * s + 2] + Ta.t[rr];
      cb[rr] = Tb.R[3 * rr + 0] * P->ls_center[3 * s + 0] + Tb.R[3 * rr + 1] * P->ls_center[3 * s + 1] + Tb.R[3 * rr + 2] * P->ls_center[3 * s + 2] + Tb.t[rr];
    }
    const double e[3] = { cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2] };
    if (P->n_ob_box > 0)
      tau = swept_closest_b_nl(ca, e, P->ob_center + 3 * o, P->ob_axis + 3 * o, P->ob_box + 12 * o, P->mesh, oq, &inside);
    else
      tau = tmx_swept_closest_to_obstacle(ca, e, P->ob_center + 3 * o, P->ob_axis + 3 * o, oq);
    for (int rr = 0; rr < 3; ++rr)
      p[rr] = ca[rr] + tau * e[rr];
  }
  const double len = tmx_contact_normal(p, oq, inside, n);
  return len - P->ls_radius[s] - P->ob_radius[o];
}

// out_min / out_pen: n x T; out_key: n x T x 3 = (sub-state i, primitive s, obstacle o) of the step's closest contact (-1: none)
template <bool HULL>
TMX_DEVFN void check_body(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, double* out_min, double* out_pen, int* out_key)
{
  TMX_SMEM(smem);
  const int tid = threadIdx.x, NT = blockDim.x;
  const int b = (int)blockIdx.x / a.chunks, c = (int)blockIdx.x % a.chunks;
  if (a.converged_only && Bt->status[b] != a.converged_code)
    return;  // (uniform over the workgroup)
  const int D = P->D, DK = P->DK, T = P->T, S = P->S, O = P->O;
  const bool seg = a.type >= 2, cast = a.type >= 3;
  const int TE = seg ? T - 1 : T;
  const long long SO = (long long)S * O;
  double* fr = smem;                                   // [fcap][DK][12]
  double* dt = fr + (size_t)a.fcap * DK * 12;           // [tile]
  double* bm = dt + a.tile;                             // [NT] block minima
  int* bi = reinterpret_cast<int*>(bm + NT);            // [NT] their items (in the tile; -1: empty block)
  int* bp = bi + NT;                                    // [NT] items of the block below the margin
  int upto = 0;
  for (int s = 0; s < S; ++s)
    upto = P->ls_link[s] > upto ? P->ls_link[s] : upto;
  const double* xb = x + (size_t)b * T * D;
  const int t0 = c * a.spc, t1 = (t0 + a.spc < T) ? t0 + a.spc : T;
  for (int t = t0; t < t1; ++t)
  {
    const size_t ot = (size_t)b * T + t;
    if (t >= TE || SO == 0)
    {
      if (tid == 0)
      {
        out_min[ot] = 1e300;
        out_pen[ot] = 0.0;
        out_key[3 * ot + 0] = out_key[3 * ot + 1] = out_key[3 * ot + 2] = -1;
      }
      continue;
    }
    const double* q0 = xb + (size_t)t * D;
    const double* q1 = seg ? q0 + D : q0;
    // sub-states of the segment: the rule of lvs_contact (the joints only; CONTINUOUS never splits)
    int cnt = seg ? 2 : 1;
    if (a.type == 2 || a.type == 4)
    {
      double d2 = 0.0;
      for (int j = 0; j < DK; ++j)
        d2 += (q1[j] - q0[j]) * (q1[j] - q0[j]);
      const double dist = sqrt(d2);
      if (dist > a.lvs)
        cnt = (int)ceil(dist / a.lvs) + 1;
      if (cnt > a.kmax || cnt < 2)  // (cnt < 2: the int conversion of a huge quotient)
        cnt = a.kmax;
    }
    const int nsub = cast ? cnt - 1 : cnt;
    const long long nit = (long long)nsub * SO;
    double cmin = 1e300, csum = 0.0;
    long long ckey = -1;
    for (long long k0 = 0; k0 < nit; k0 += a.tile)
    {
      const long long k1 = (k0 + a.tile < nit) ? k0 + a.tile : nit;
      const int ia = (int)(k0 / SO), ib = (int)((k1 - 1) / SO);
      const int ns = ib - ia + 1 + (cast ? 1 : 0);
      // ---- phase 1: the link frames of sub-states ia .. ia + ns - 1
      for (int st = tid; st < ns; st += NT)
      {
        const int i = ia + st;
        check_link_frames(P, [=](int j) { return seg ? lin_spaced_at(cnt, q0[j], q1[j], i) : q0[j]; }, upto, fr + (size_t)st * DK * 12);
      }
      TMX_SYNC();
      // ---- phase 2: the distance of every item of the tile
      for (long long k = k0 + tid; k < k1; k += NT)
      {
        const int i = (int)(k / SO);
        const int rem = (int)(k - (long long)i * SO);
        const int s = rem / O, o = rem - s * O;
        const double* fa = fr + ((size_t)(i - ia) * DK + P->ls_link[s]) * 12;
        Tf3 Ta;
        check_load_frame(fa, Ta);
        double d;
        if (cast)
        {
          Tf3 Tb;
          check_load_frame(fa + (size_t)DK * 12, Tb);
          d = check_swept_distance<HULL>(P, Ta, Tb, s, o);
        }
        else
        {
          double n[3], pw[3];
          d = contact_distance_at<HULL>(P, Ta, s, o, n, pw);
        }
        dt[k - k0] = d;
      }
      TMX_SYNC();
      // ---- phase 3: block scan by every thread, ordered fold by thread 0
      const int n = (int)(k1 - k0), per = (n + NT - 1) / NT;
      {
        const int lo = tid * per, hi = (lo + per < n) ? lo + per : n;
        double lm = 1e300;
        int li = -1, lp = 0;
        for (int j = lo; j < hi; ++j)
        {
          const double d = dt[j];
          if (li < 0 || d < lm)
          {
            lm = d;
            li = j;
          }
          lp += (a.margin - d > 0.0) ? 1 : 0;
        }
        bm[tid] = lm;
        bi[tid] = li;
        bp[tid] = lp;
      }
      TMX_SYNC();
      if (tid == 0)
        for (int blk = 0; blk < NT; ++blk)
        {
          if (bi[blk] >= 0 && (ckey < 0 || bm[blk] < cmin))
          {
            cmin = bm[blk];
            ckey = k0 + bi[blk];
          }
          if (bp[blk] > 0)
          {
            const int lo = blk * per, hi = (lo + per < n) ? lo + per : n;
            for (int j = lo; j < hi; ++j)
            {
              const double h = a.margin - dt[j];
              if (h > 0.0)
                csum += h;
            }
          }
        }
      TMX_SYNC();  // (the next tile overwrites the tables)
    }
    if (tid == 0)
    {
      const int i = (int)(ckey / SO);
      const int rem = (int)(ckey - (long long)i * SO);
      out_min[ot] = cmin;
      out_pen[ot] = csum;
      out_key[3 * ot + 0] = i;
      out_key[3 * ot + 1] = rem / O;
      out_key[3 * ot + 2] = rem - (rem / O) * O;
    }
  }
}
TMX_KERNEL_LB(256) k_check_trajectories(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, double* out_min, double* out_pen, int* out_key)
{
  check_body<false>(P, Bt, x, a, out_min, out_pen, out_key);
}
TMX_KERNEL_LB(256) k_check_trajectories_hull(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, double* out_min, double* out_pen, int* out_key)
{
  check_body<true>(P, Bt, x, a, out_min, out_pen, out_key);
}

// the closest contact of every trajectory over its per-step results: one thread per trajectory, steps ascending (strict <: the lowest
// step wins a tie, inside a step k_check_trajectories already kept the lowest (i, s, o))
TMX_KERNEL k_check_worst(int n, int T, const double* step_min, const int* step_key, tmx_check_worst* worst)
{
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= n)
    return;
  tmx_check_worst w;
  w.min_distance = 1e300;
  w.step = w.primitive = w.obstacle = w.substate = -1;
  for (int t = 0; t < T; ++t)
  {
    const size_t ot = (size_t)b * T + t;
    if (step_key[3 * ot] >= 0 && (w.step < 0 || step_min[ot] < w.min_distance))
    {
      w.min_distance = step_min[ot];
      w.step = t;
      w.substate = step_key[3 * ot + 0];
      w.primitive = step_key[3 * ot + 1];
      w.obstacle = step_key[3 * ot + 2];
    }
  }
  worst[b] = w;
}

// K7 per query over the FREE converged seeds (tmx_best_trajectories_checked): the rule and the reduction of k_argmin_queries, restricted
// to seeds whose per-step minima (written by k_check_trajectories for the converged seeds) are all >= margin.  out_clear[q] = the
// winner's smallest distance (1e300: no winner, or a scene without contacts).  LDS: 16 doubles + 17 ints.
TMX_KERNEL k_argmin_queries_checked(const DevBatch* Bt, int converged_code, int S, int NX, int T, double margin, const double* step_min,
                                    double* out_cost, long long* out_index, double* out_clear, double* x_out)
{
  TMX_SMEM(smem);
  const int q = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  double bc = 1e300;
  int bi = -1;
  for (int s = tid; s < S; s += NT)  // (ascending indices per thread: the strict comparison keeps the lowest index of equal costs)
  {
    const int b = q * S + s;
    if (Bt->status[b] != converged_code)
      continue;
    double md = 1e300;
    for (int t = 0; t < T; ++t)
      md = step_min[(size_t)b * T + t] < md ? step_min[(size_t)b * T + t] : md;
    if (md >= margin && Bt->total_cost[b] < bc)
    {
      bc = Bt->total_cost[b];
      bi = b;
    }
  }
  [[maybe_unused]] double* wc = smem;           // [16] the waves' costs
  int* wi = reinterpret_cast<int*>(smem + 16);  // [16] the waves' indices, [16] = the winner
#if TMX_IS_DEVICE
  if (NT > 1)
  {
    const int lane = tid & 63, wv = tid >> 6, nw = (NT + 63) >> 6;
    argmin_wave(bc, bi);
    if (lane == 0)
    {
      wc[wv] = bc;
      wi[wv] = bi;
    }
    TMX_SYNC();
    if (wv == 0)
    {
      bc = lane < nw ? wc[lane] : 1e300;
      bi = lane < nw ? wi[lane] : -1;
      argmin_wave(bc, bi);
    }
  }
#endif
  if (tid == 0)
  {
    double md = 1e300;
    if (bi >= 0)
      for (int t = 0; t < T; ++t)
        md = step_min[(size_t)bi * T + t] < md ? step_min[(size_t)bi * T + t] : md;
    out_cost[q] = bc;
    out_index[q] = bi;
    out_clear[q] = md;
    wi[16] = bi;
  }
  if (x_out == nullptr)
    return;
  TMX_SYNC();
  const int win = wi[16];
  const double* src = Bt->x + (size_t)(win < 0 ? 0 : win) * NX;
  for (int v = tid; v < NX; v += NT)
    x_out[(size_t)q * NX + v] = win < 0 ? 0.0 : src[v];
}
