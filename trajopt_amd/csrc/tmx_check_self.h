// tmx_check_self.h — self-collision side of the batched trajectory check (tmx_check_self_trajectories and the fold into
// tmx_best_trajectories_checked).
//
// The obstacle check (tmx_check.h) measures link primitives against obstacles; here a contact is (step t, sub-state or swept
// sub-segment i, PRIMITIVE PAIR p = (sa, sb)) with sa, sb on two different links.  The pair table pp[PP][2] is expanded on the host
// from the link pairs of tmx_check_set_link_pairs (link pair, then sa, then sb, all ascending) and is an argument of the kernels:
// DevProblem does not know it, and no SQP / QP kernel can reach it.
//
// Distance of a pair:
//   discrete types  both primitives at the frames of the same sub-state; the cores are a point (sphere) or a segment (capsule), the
//                   closest points come from tmx_link_closest_to_obstacle with b's world core in the place of the obstacle
//   cast types      each primitive swept between sub-states i and i + 1 of ITS OWN link (the link side of check_swept_distance on
//                   both sides): two swept spheres are two segment cores
//   hull on a side  tmx_gjk_epa on two tmx_cvx: kind 4 / 5 for a (swept) hull, kind 0 / 1 for a point / segment core
// and both radii are subtracted.
//
// k_check_self has the three-phase shape of check_body, items k = i * PP + p: one thread per sub-state leaves the link frames in LDS,
// the items strided over the threads fill an LDS distance table, every thread scans a block and thread 0 folds the blocks in ascending
// order.  So every result is the left fold over the ascending items whatever the number of threads, chunks or tiles.  No atomics, no
// hand-off between workgroups.  The frame table is read through address-space-3 pointers, 16 bytes at a time (a frame is 96 bytes
// at a multiple of 96: six ds_read_b128).
#pragma once
#include "tmx_check.h"

// frame st * DK + link of the LDS table as 6 x 16 bytes (the host build has no address spaces: check_load_frame)
#if !TMX_IS_DEVICE
typedef double check_self_lds_d;
#define check_self_load_frame check_load_frame
#else
typedef tmx_lds_d check_self_lds_d;
TMX_DEVFN void check_self_load_frame(const tmx_lds_d* f, Tf3& T)
{
  const tmx_lds_d2* f2 = (const tmx_lds_d2*)f;
  const tmx_d2 a = f2[0], b = f2[1], c = f2[2], d = f2[3], e = f2[4], g = f2[5];
  T.R[0] = a.x;
  T.R[1] = a.y;
  T.R[2] = b.x;
  T.R[3] = b.y;
  T.R[4] = c.x;
  T.R[5] = c.y;
  T.R[6] = d.x;
  T.R[7] = d.y;
  T.R[8] = e.x;
  T.t[0] = e.y;
  T.t[1] = g.x;
  T.t[2] = g.y;
}
#endif
// world position of the link-frame point v of a link placed at L (the operation order of contact_distance_at)
TMX_DEVFN void check_self_point(const Tf3& L, const double* v, double out[3])
{
  for (int r = 0; r < 3; ++r)
    out[r] = L.R[3 * r + 0] * v[0] + L.R[3 * r + 1] * v[1] + L.R[3 * r + 2] * v[2] + L.t[r];
}
TMX_DEVFN void check_self_dir(const Tf3& L, const double* v, double out[3])
{
  for (int r = 0; r < 3; ++r)
    out[r] = L.R[3 * r + 0] * v[0] + L.R[3 * r + 1] * v[1] + L.R[3 * r + 2] * v[2];
}

// primitive s of a link placed at L0 (swept to L1 when cast) as a convex set: a hull keeps its vertex cloud (kind 4 / 5), a sphere or
// capsule its core (kind 0 / 1; a swept sphere is the segment of its centres); buf = 6 doubles the set points into
TMX_DEVFN void check_self_cvx(const DevProblem* P, int s, const Tf3& L0, const Tf3& L1, bool cast, tmx_cvx* C, double* buf)
{
  C->b = 0;
  C->n = 0;
  if (P->n_ls_hull > 0 && P->ls_hull[2 * s + 1] > 0)
  {
    C->kind = cast ? 5 : 4;
    C->a = P->hull + 3 * P->ls_hull[2 * s];
    C->n = P->ls_hull[2 * s + 1];
    for (int k = 0; k < 9; ++k)
    {
      C->R[k] = L0.R[k];
      C->R2[k] = L1.R[k];
    }
    for (int k = 0; k < 3; ++k)
    {
      C->t[k] = L0.t[k];
      C->t2[k] = L1.t[k];
    }
    return;
  }
  check_self_point(L0, P->ls_center + 3 * s, buf);
  if (cast)
  {
    double c1[3];
    check_self_point(L1, P->ls_center + 3 * s, c1);
    for (int r = 0; r < 3; ++r)
      buf[3 + r] = c1[r] - buf[r];
  }
  else
    check_self_dir(L0, P->ls_axis + 3 * s, buf + 3);
  C->a = buf;
  C->b = buf + 3;
  C->kind = (buf[3] * buf[3] + buf[4] * buf[4] + buf[5] * buf[5]) > TMX_GM_EPS ? 1 : 0;
}
// a pair with a hull on a side: GJK / EPA (cold, a few KB of private arrays: out of line on the device, as hull_closest_nl)
#if TMX_IS_DEVICE && TMX_IS_GCN
__device__ __attribute__((noinline)) static int check_self_gjk_nl(const tmx_cvx* A, const tmx_cvx* B, double* p, double* q) { return tmx_gjk_epa(A, B, p, q); }
#else
#define check_self_gjk_nl tmx_gjk_epa
#endif

// signed distance of the primitive pair (sa, sb): link of sa at A0 (swept to A1), link of sb at B0 (swept to B1)
template <bool HULL>
TMX_DEVFN double check_self_distance(const DevProblem* P, const Tf3& A0, const Tf3& A1, const Tf3& B0, const Tf3& B1, bool cast, int sa, int sb)
{
  double p[3], q[3], n[3];
  int inside = 0;
  bool hull = false;
  if constexpr (HULL)
    hull = P->n_ls_hull > 0 && (P->ls_hull[2 * sa + 1] > 0 || P->ls_hull[2 * sb + 1] > 0);
  if (hull)
  {
    tmx_cvx A, B;
    double ba[6], bb[6];
    check_self_cvx(P, sa, A0, A1, cast, &A, ba);
    check_self_cvx(P, sb, B0, B1, cast, &B, bb);
    inside = check_self_gjk_nl(&A, &B, p, q);
  }
  else
  {
    double ca[3], cb[3], ea[3], eb[3];
    check_self_point(A0, P->ls_center + 3 * sa, ca);
    check_self_point(B0, P->ls_center + 3 * sb, cb);
    if (cast)
    {
      // two swept centres: the two-segment problem of the cast branch, b's sweep in the place of the capsule obstacle's axis
      double a1[3], b1[3];
      check_self_point(A1, P->ls_center + 3 * sa, a1);
      check_self_point(B1, P->ls_center + 3 * sb, b1);
      for (int r = 0; r < 3; ++r)
      {
        ea[r] = a1[r] - ca[r];
        eb[r] = b1[r] - cb[r];
      }
      const double tau = tmx_swept_closest_to_obstacle(ca, ea, cb, eb, q);
      for (int r = 0; r < 3; ++r)
        p[r] = ca[r] + tau * ea[r];
    }
    else
    {
      bool cap_a = false;
      eb[0] = eb[1] = eb[2] = 0.0;
      if (P->n_ls_capsule > 0)
      {
        const double* xa = P->ls_axis + 3 * sa;
        cap_a = xa[0] != 0.0 || xa[1] != 0.0 || xa[2] != 0.0;
        check_self_dir(A0, xa, ea);
        check_self_dir(B0, P->ls_axis + 3 * sb, eb);
      }
      tmx_link_closest_to_obstacle(ca, cap_a ? ea : nullptr, cb, eb, p, q);
    }
  }
  const double len = tmx_contact_normal(p, q, inside, n);
  return len - P->ls_radius[sa] - P->ls_radius[sb];
}

// pp: PP x 2 = (primitive a, primitive b); out_min / out_pen: n x T; out_key: n x T x 2 = (sub-state i, primitive pair p) of the
// step's closest contact (-1: none).  CheckArgs as for check_body with PP in the place of S * O.
template <bool HULL>
TMX_DEVFN void check_self_body(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, const int* pp, int PP, double* out_min,
                               double* out_pen, int* out_key)
{
  TMX_SMEM(smem);
  const int tid = threadIdx.x, NT = blockDim.x;
  const int b = (int)blockIdx.x / a.chunks, c = (int)blockIdx.x % a.chunks;
  if (a.converged_only && Bt->status[b] != a.converged_code)
    return;  // (uniform over the workgroup)
  const int D = P->D, DK = P->DK, T = P->T, S = P->S;
  const bool seg = a.type >= 2, cast = a.type >= 3;
  const int TE = seg ? T - 1 : T;
  double* fr = smem;                                   // [fcap][DK][12]
  check_self_lds_d* const frl = (check_self_lds_d*)smem;             // (the same table for the reads of phase 2)
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
    if (t >= TE || PP == 0)
    {
      if (tid == 0)
      {
        out_min[ot] = 1e300;
        out_pen[ot] = 0.0;
        out_key[2 * ot + 0] = out_key[2 * ot + 1] = -1;
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
    const long long nit = (long long)nsub * PP;
    double cmin = 1e300, csum = 0.0;
    long long ckey = -1;
    for (long long k0 = 0; k0 < nit; k0 += a.tile)
    {
      const long long k1 = (k0 + a.tile < nit) ? k0 + a.tile : nit;
      const int ia = (int)(k0 / PP), ib = (int)((k1 - 1) / PP);
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
        const int i = (int)(k / PP);
        const int p = (int)(k - (long long)i * PP);
        const int sa = pp[2 * p], sb = pp[2 * p + 1];
        const check_self_lds_d* fa = frl + ((size_t)(i - ia) * DK + P->ls_link[sa]) * 12;
        const check_self_lds_d* fb = frl + ((size_t)(i - ia) * DK + P->ls_link[sb]) * 12;
        Tf3 A0, B0;
        check_self_load_frame(fa, A0);
        check_self_load_frame(fb, B0);
        double d;
        if (cast)
        {
          Tf3 A1, B1;
          check_self_load_frame(fa + (size_t)DK * 12, A1);
          check_self_load_frame(fb + (size_t)DK * 12, B1);
          d = check_self_distance<HULL>(P, A0, A1, B0, B1, true, sa, sb);
        }
        else
          d = check_self_distance<HULL>(P, A0, A0, B0, B0, false, sa, sb);
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
      const int i = (int)(ckey / PP);
      out_min[ot] = cmin;
      out_pen[ot] = csum;
      out_key[2 * ot + 0] = i;
      out_key[2 * ot + 1] = (int)(ckey - (long long)i * PP);
    }
  }
}
TMX_KERNEL_LB(256) k_check_self(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, const int* pp, int PP, double* out_min,
                                double* out_pen, int* out_key)
{
  check_self_body<false>(P, Bt, x, a, pp, PP, out_min, out_pen, out_key);
}
TMX_KERNEL_LB(256) k_check_self_hull(const DevProblem* P, const DevBatch* Bt, const double* x, CheckArgs a, const int* pp, int PP, double* out_min,
                                     double* out_pen, int* out_key)
{
  check_self_body<true>(P, Bt, x, a, pp, PP, out_min, out_pen, out_key);
}

// the closest self-contact of every trajectory over its per-step results: one thread per trajectory, steps ascending (strict <: the
// lowest step wins a tie, inside a step k_check_self already kept the lowest (i, p))
TMX_KERNEL k_check_self_worst(int n, int T, const double* step_min, const int* step_key, const int* pp, tmx_check_self_worst* worst)
{
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= n)
    return;
  tmx_check_self_worst w;
  w.min_distance = 1e300;
  w.step = w.primitive_a = w.primitive_b = w.substate = -1;
  for (int t = 0; t < T; ++t)
  {
    const size_t ot = (size_t)b * T + t;
    if (step_key[2 * ot] >= 0 && (w.step < 0 || step_min[ot] < w.min_distance))
    {
      w.min_distance = step_min[ot];
      w.step = t;
      w.substate = step_key[2 * ot + 0];
      w.primitive_a = pp[2 * step_key[2 * ot + 1]];
      w.primitive_b = pp[2 * step_key[2 * ot + 1] + 1];
    }
  }
  worst[b] = w;
}

// step_min[b][t] = min(step_min[b][t], self_min[b][t]) for the seeds the check kernels wrote (tmx_best_trajectories_checked runs both
// with converged_only: the rows of the other seeds hold nothing and k_argmin_queries_checked never reads them).  A minimum does not round.
TMX_KERNEL k_check_fold_min(const DevBatch* Bt, int converged_code, int n, int T, const double* self_min, double* step_min)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)n * T)
    return;
  if (Bt->status[k / T] != converged_code)
    return;
  step_min[k] = self_min[k] < step_min[k] ? self_min[k] : step_min[k];
}
