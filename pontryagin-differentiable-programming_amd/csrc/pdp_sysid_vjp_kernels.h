// pdp_sysid_vjp_kernels.h - the SysID rollout as a vector-Jacobian product (include/pdp_hip_sysid_vjp.h): the gradient of ANY scalar loss L(x_0 .. x_T) of a rollout
// x_{t+1} = f(x_t, u_t, theta) with respect to theta and x_0 from the cotangents g_t = dL/dx_t, by the adjoint (costate) sweep
//     lam_T = g_T ;   t = T-1 .. 0 :   dL/dtheta += E_t' lam_{t+1} ,   lam_t = g_t + F_t' lam_{t+1} ;   dL/dx_0 = lam_0
// (F_t = df/dx, E_t = df/dtheta at (x_t, u_t, theta): the models' `path` group).  O(T (n^2 + n p)) and nothing larger than a vector per step, where the forward
// sensitivities X_{t+1} = F_t X_t + E_t of sysid_step_kernel cost O(T n^2 p) and serve one loss.  Instantiated for PDP_KIND_SYSID only (pdp_model.hip).
// With the inputs (include/pdp_hip_sysid_vjp_u.h): the same sweep also gives dL/du_t = G_t' lam_{t+1} (G_t = df/du: the models' `pathu` group) - sysid_vjp_u_kernel,
// a kernel of its own below sysid_vjp_kernel.  (One force-inlined body with a compile-time switch under both was built first: the wrapper did not compile to the
// instructions sysid_vjp_kernel had - the scalar code of the chunk arithmetic came out in another order - so that kernel keeps its own text: DESIGN.md section 4.1k.)
#pragma once
#include "pdp_model_kernels.h"
#include "pdp_sweep_pool.h"

namespace pdp {

// A sweep kernel on SysidVjpPool (pdp_sweep_pool.h: the block, the rows, the structure), on the GIVEN trajectory x (what sysid_integrate_kernel wrote): no rollout
// here.  The chunks are visited last to first.  Per chunk: lane tl loads x_t, u_t, g_t of step t = t0 + tl and evaluates the model's path group through a PackedSink
// into pool row tl; then the serial sweep over the chunk's steps.  In the sweep lane i < NX owns lam[i] and reads column i of F_t, the lane of parameter j = lane + 64 q owns its accumulator and reads column j of E_t; lam_{t+1}[k] reaches all of them
// as a scalar (v_readlane of its owner's register), so the recursion's chain holds no LDS write / read pair and no global read: the pool reads of a step do not depend
// on lam.  The E_t' lam_{t+1} accumulation stays in the step loop (it shares the broadcast lam_{t+1}[k] with the recursion and does not feed it).
// theta is read through its (uniform) pointer - scalar loads, no register per parameter, whatever p.  No masking, no status word: a NaN anywhere in this trajectory's
// x, u, theta or g reaches this trajectory's outputs only.
template <class Mdl>
__global__ void __launch_bounds__(64) sysid_vjp_kernel(int B, int T, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ theta,
                                                        int tb, const double* __restrict__ gx, double* __restrict__ grad_theta, double* __restrict__ grad_x0, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP, NQ = NP > 0 ? (NP + 63) / 64 : 1;
    using Pool = SysidVjpPool<Mdl>;
    constexpr int NC = Pool::NC, GX = Pool::GX, STRIDE = Pool::STRIDE;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* blk = lds;
    double* pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* th = theta + (int64_t)b * tb;
    double pc[Mdl::NPC];
    Mdl::precompute(th, pc);
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* ub = u + (int64_t)b * T * NU;
    const double* gb = gx + (int64_t)b * (T + 1) * NX;
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    // per-lane pool offsets (o) and row multipliers (m): column `lane` of F, g_t[lane], column lane + 64 q of E
    int fo[NX], fm[NX], eo[NQ][NX], em[NQ][NX], go = 0, gm = 0;
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(0, k * NX + lane) : -1, fo[k], fm[k]);
#pragma unroll
        for (int q = 0; q < NQ; ++q) pool_enc<NC, STRIDE>(lane + 64 * q < NP ? Mdl::path_code(1, k * NP + lane + 64 * q) : -1, eo[q][k], em[q][k]);
    }
    if (lane < NX) { go = NC + GX + lane; gm = STRIDE; }
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    double lam = lane < NX ? gb[(int64_t)T * NX + lane] : 0.0;             // lam_T = g_T
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = nchunk - 1; c >= 0; --c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        wave_lds_sync();
        if (lane < cnt) {
            const int t = t0 + lane;
            double xc[NX], uc[NU];
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) { xc[i] = xb[t * NX + i]; row[GX + i] = gb[t * NX + i]; }
#pragma unroll
            for (int i = 0; i < NU; ++i) uc[i] = ub[t * NU + i];
            PackedSink s{row};
            Mdl::eval_path(xc, uc, nullptr, th, pc, s);
        }
        wave_lds_sync();
        for (int tl = cnt - 1; tl >= 0; --tl) {
            double m_new = blk[go + tl * gm];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double lk = readlane_f64(lam, k);
                m_new += blk[fo[k] + tl * fm[k]] * lk;
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += blk[eo[q][k] + tl * em[q][k]] * lk;
            }
            lam = m_new;
        }
    }
    if (grad_theta) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) { const int j = lane + 64 * q; if (j < NP) grad_theta[(int64_t)b * NP + j] = acc[q]; }
    }
    if (grad_x0 && lane < NX) grad_x0[(int64_t)b * NX + lane] = lam;
}

// sysid_vjp_kernel with the gradient with respect to the inputs, on SysidVjpUPool.  The lane-per-step pass also evaluates the `pathu` group (G_t) behind the path entries of its row.  In
// the sweep a lane owns the columns c = lane + 64 q of the n x (p + m) matrix [E_t | G_t]: c < p accumulates over the horizon as above (same products, same order),
// p <= c < p + m is one step's G_t' lam_{t+1} - behind the k loop of step tl its lane stores the sum into the row's staging slot and restarts from 0.0 (a select: the
// products run in every lane).  No read and no product more in the loop than a slot of E columns costs, and nothing on the recursion's chain.  After the chunk's sweep lane
// tl copies its row's m values to grad_u[b][t0 + tl] (adjacent lanes, adjacent 8 m bytes); the sync at the top of the next chunk protects the rows.  Every grad_u[b][t]
// is written exactly once and never read.  grad_u is never NULL here: without it the host routine launches the kernel above.
template <class Mdl>
__global__ void __launch_bounds__(64) sysid_vjp_u_kernel(int B, int T, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ theta,
                                                          int tb, const double* __restrict__ gx, double* __restrict__ grad_theta, double* __restrict__ grad_x0,
                                                          double* __restrict__ grad_u, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP, NQ = (NP + NU + 63) / 64;
    using Pool = SysidVjpUPool<Mdl>;
    constexpr int NC = Pool::NC, GX = Pool::GX, SU = Pool::SU, STRIDE = Pool::STRIDE;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* blk = lds;
    double* pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* th = theta + (int64_t)b * tb;
    double pc[Mdl::NPCU];
    Mdl::precompute_u(th, pc);                     // precompute's values and, behind them, those that `pathu` alone reads
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* ub = u + (int64_t)b * T * NU;
    const double* gb = gx + (int64_t)b * (T + 1) * NX;
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    for (int i_ = lane; i_ < Mdl::PATHU_NCONST; i_ += 64) blk[1 + Mdl::PATH_NCONST + i_] = Mdl::pathu_const(i_);
    // per-lane pool offsets (o) and row multipliers (m): column `lane` of F, g_t[lane], column lane + 64 q of [E | G]
    int fo[NX], fm[NX], eo[NQ][NX], em[NQ][NX], go = 0, gm = 0;
    // a G entry's variable sits behind the path entries of the row, its constant behind the path constants of the block
    auto encu = [&](int code, int& o, int& m) { pool_enc<NC, STRIDE>(code >= 0 ? Mdl::PATH_NVAR + code : (code == -1 ? -1 : code - Mdl::PATH_NCONST), o, m); };
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(0, k * NX + lane) : -1, fo[k], fm[k]);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = lane + 64 * q;
            if (c >= NP && c < NP + NU) encu(Mdl::pathu_code(0, k * NU + (c - NP)), eo[q][k], em[q][k]);
            else pool_enc<NC, STRIDE>(c < NP ? Mdl::path_code(1, k * NP + c) : -1, eo[q][k], em[q][k]);
        }
    }
    if (lane < NX) { go = NC + GX + lane; gm = STRIDE; }
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    double lam = lane < NX ? gb[(int64_t)T * NX + lane] : 0.0;             // lam_T = g_T
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = nchunk - 1; c >= 0; --c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        wave_lds_sync();
        if (lane < cnt) {
            const int t = t0 + lane;
            double xc[NX], uc[NU];
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) { xc[i] = xb[t * NX + i]; row[GX + i] = gb[t * NX + i]; }
#pragma unroll
            for (int i = 0; i < NU; ++i) uc[i] = ub[t * NU + i];
            PackedSink s{row}, su{row + Mdl::PATH_NVAR};
            Mdl::eval_path(xc, uc, nullptr, th, pc, s);
            Mdl::eval_pathu(xc, uc, nullptr, th, pc, su);
        }
        wave_lds_sync();
        for (int tl = cnt - 1; tl >= 0; --tl) {
            double m_new = blk[go + tl * gm];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double lk = readlane_f64(lam, k);
                m_new += blk[fo[k] + tl * fm[k]] * lk;
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += blk[eo[q][k] + tl * em[q][k]] * lk;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (64 * q + 63 >= NP && 64 * q < NP + NU) {               // (known per slot once unrolled: some lane of it holds a G column)
                    const int cu = lane + 64 * q - NP;
                    const bool isu = cu >= 0 && cu < NU;
                    if (isu) pool[tl * STRIDE + SU + cu] = acc[q];         // dL/du_t[cu] = column cu of G_t . lam_{t+1}
                    acc[q] = isu ? 0.0 : acc[q];
                }
            }
            lam = m_new;
        }
        wave_lds_sync();
        if (lane < cnt) {
            const double* stage = pool + lane * STRIDE + SU;
            double* out = grad_u + ((int64_t)b * T + t0 + lane) * NU;
#pragma unroll
            for (int j = 0; j < NU; ++j) out[j] = stage[j];
        }
    }
    if (grad_theta) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) { const int j = lane + 64 * q; if (j < NP) grad_theta[(int64_t)b * NP + j] = acc[q]; }
    }
    if (grad_x0 && lane < NX) grad_x0[(int64_t)b * NX + lane] = lam;
}

}  // namespace pdp
