// pdp_sysid_vjp_kernels.h - the SysID rollout as a vector-Jacobian product (include/pdp_hip_sysid_vjp.h): the gradient of ANY scalar loss L(x_0 .. x_T) of a rollout
// x_{t+1} = f(x_t, u_t, theta) with respect to theta and x_0 from the cotangents g_t = dL/dx_t, by the adjoint (costate) sweep
//     lam_T = g_T ;   t = T-1 .. 0 :   dL/dtheta += E_t' lam_{t+1} ,   lam_t = g_t + F_t' lam_{t+1} ;   dL/dx_0 = lam_0
// (F_t = df/dx, E_t = df/dtheta at (x_t, u_t, theta): the models' `path` group).  O(T (n^2 + n p)) and nothing larger than a vector per step, where the forward
// sensitivities X_{t+1} = F_t X_t + E_t of sysid_step_kernel cost O(T n^2 p) and serve one loss.  Instantiated for PDP_KIND_SYSID only (pdp_model.hip).
#pragma once
#include "pdp_model_kernels.h"

namespace pdp {

// a pool row of the kernel below: the packed variable entries of (F_t, E_t), then the NX cotangents g_t
template <class Mdl> constexpr int sysid_vjp_stride() { return (Mdl::PATH_NVAR + Mdl::NX) | 1; }
// doubles of dynamic LDS: [0.0 | constants | rows x stride], rounded up to 16 bytes
template <class Mdl>
__host__ __device__ inline int sysid_vjp_slice(int rows) { return (1 + Mdl::PATH_NCONST + rows * sysid_vjp_stride<Mdl>() + 1) & ~1; }
// Pool rows (time steps per lane-parallel Jacobian pass).  The generated CHUNK while a CU holds at most one trajectory per SIMD; a larger batch gets a pool of at most
// 2400 doubles (18.75 KB: with the constants and the allocation granularity an eighth of the CU's 160 KB), so that two workgroups per SIMD are resident and fill each
// other's waits - the rule of sysid_rows.  The rule reads the row stride alone: runtime.ModelLib.sysid_vjp_rows restates it.  The result bits do not depend on it: the
// sweep visits the steps in the same order whatever the pass they were evaluated in.
template <class Mdl>
__host__ inline int sysid_vjp_rows(int B, int cus) {
    if (B <= 4 * cus) return Mdl::CHUNK;
    const int fit = 2400 / sysid_vjp_stride<Mdl>();
    return fit >= 4 ? (fit < Mdl::CHUNK ? fit : Mdl::CHUNK) : Mdl::CHUNK;
}

// One wavefront per trajectory on the GIVEN trajectory x (what sysid_integrate_kernel wrote): no rollout here.  The horizon is cut into chunks of equal length <= CH,
// visited last to first (cp_step_adjoint_kernel's structure).  Per chunk: lane tl loads x_t, u_t, g_t of step t = t0 + tl and evaluates the model's path group through a
// PackedSink into pool row tl (structural zeros read blk[0] = 0.0, constants the block behind it); then the serial sweep over the chunk's steps.  In the sweep lane
// i < NX owns lam[i] and reads column i of F_t, the lane of parameter j = lane + 64 q owns its accumulator and reads column j of E_t; lam_{t+1}[k] reaches all of them
// as a scalar (v_readlane of its owner's register), so the recursion's chain holds no LDS write / read pair and no global read: the pool reads of a step do not depend
// on lam.  The E_t' lam_{t+1} accumulation stays in the step loop (it shares the broadcast lam_{t+1}[k] with the recursion and does not feed it).
// theta is read through its (uniform) pointer - scalar loads, no register per parameter, whatever p.  No masking, no status word: a NaN anywhere in this trajectory's
// x, u, theta or g reaches this trajectory's outputs only.
template <class Mdl>
__global__ void __launch_bounds__(64) sysid_vjp_kernel(int B, int T, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ theta,
                                                        int tb, const double* __restrict__ gx, double* __restrict__ grad_theta, double* __restrict__ grad_x0, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP, NQ = NP > 0 ? (NP + 63) / 64 : 1;
    constexpr int NC = 1 + Mdl::PATH_NCONST, GX = Mdl::PATH_NVAR, STRIDE = sysid_vjp_stride<Mdl>();
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
    auto enc = [&](int code, int& o, int& m) { if (code >= 0) { o = NC + code; m = STRIDE; } else { o = (code == -1) ? 0 : 1 + (-2 - code); m = 0; } };
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        enc(lane < NX ? Mdl::path_code(0, k * NX + lane) : -1, fo[k], fm[k]);
#pragma unroll
        for (int q = 0; q < NQ; ++q) enc(lane + 64 * q < NP ? Mdl::path_code(1, k * NP + lane + 64 * q) : -1, eo[q][k], em[q][k]);
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
                const double lk = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lam), k), __builtin_amdgcn_readlane(__double2loint(lam), k));
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

}  // namespace pdp
