// pdp_sysid_jvp_kernels.h - the SysID rollout as a Jacobian-vector product (include/pdp_hip_sysid_jvp.h): the tangent of a rollout x_{t+1} = f(x_t, u_t, theta) along a
// direction (d_theta, d_x0, d_u) by the forward (tangent) sweep
//     dx_0 given ;   t = 0 .. T-1 :   dx_{t+1} = F_t dx_t + E_t d_theta + G_t du_t
// (F_t = df/dx, E_t = df/dtheta: the models' `path` group; G_t = df/du: their `pathu` group) - the other half of sysid_vjp_kernel (pdp_sysid_vjp_kernels.h), the same
// O(T (n^2 + n p)) and the same pool row.  With both a Gauss-Newton product J' J v of any residual of the rollout is two launches whatever p is.  Instantiated for
// PDP_KIND_SYSID only (pdp_model.hip).  DESIGN.md section 4.1l.
#pragma once
#include "pdp_sysid_vjp_kernels.h"

namespace pdp {

// Sinks of the lane-per-step pass.  SysID groups are generated without dedup: variable entry K of a group is ONE matrix position, known at compile time (PATH_MAT[K],
// PATH_OFF[K]).  An entry of F goes to the pool row (the sweep reads it); an entry of E is folded into the forcing term w[i] += E[i][j] d_theta[j] where it is
// produced and never reaches LDS.  d_theta is read through its uniform pointer (`has` false: +0.0 in its place, a scalar select).
template <class Mdl> struct JvpPathSink {
    double* row;
    double* w;
    const double* dth;
    bool has;
    template <int K> PDP_DEV void put(double v) {
        if constexpr (Mdl::PATH_MAT[K] == 0) row[K] = v;
        else {
            constexpr int off = Mdl::PATH_OFF[K], i = off / Mdl::NP, j = off % Mdl::NP;
            w[i] += v * (has ? dth[j] : 0.0);
        }
    }
};
// ... and of G: w[i] += G[i][j] du_t[j]
template <class Mdl> struct JvpPathuSink {
    double* w;
    const double* du;
    template <int K> PDP_DEV void put(double v) {
        constexpr int off = Mdl::PATHU_OFF[K], i = off / Mdl::NU, j = off % Mdl::NU;
        w[i] += v * du[j];
    }
};

// sysid_vjp_kernel's structure and pool (SysidVjpPool, pdp_sweep_pool.h) run forwards on the GIVEN trajectory x: the chunks are visited first to last.  Per chunk lane tl evaluates the model's groups at step t = t0 + tl: the entries of F_t go to pool row tl, and the forcing term w_t = E_t d_theta + G_t du_t -
// which does not depend on the recursion - is summed there and then, entry by entry as eval_path produces it (constant entries from a compile-time loop over the codes),
// and stored in the row's n slots behind the packed entries (where the vjp kernel keeps the cotangents).  Its cost is the number of
// structurally non-zero entries of E and G.  Then the serial sweep: lane i < NX owns dx[i] and reads ROW i of F_t through offset / multiplier pairs formed once;
// dx_t[k] reaches it as a scalar (v_readlane of its owner's register), so the chain holds no LDS write / read pair, no wait on a store and no global read.  Each step's
// dx_{t+1} is stored directly to d_x[b][t+1] (n adjacent doubles, one store; nothing waits for it).  WU: with d_u (never NULL then) - `pathu` is evaluated only there.
// d_theta / d_x0 NULL: +0.0.  No masking, no status word: a NaN in this trajectory's x, u, theta or tangents reaches this trajectory's d_x only.
template <class Mdl, bool WU>
__global__ void __launch_bounds__(64) sysid_jvp_kernel(int B, int T, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ theta,
                                                        int tb, const double* __restrict__ d_theta, int dtb, const double* __restrict__ d_x0,
                                                        const double* __restrict__ d_u, double* __restrict__ d_x, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP;
    using Pool = SysidVjpPool<Mdl>;
    constexpr int NC = Pool::NC, GX = Pool::GX, STRIDE = Pool::STRIDE;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* blk = lds;
    double* pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* th = theta + (int64_t)b * tb;
    const bool has_dth = d_theta != nullptr;
    const double* dth = has_dth ? d_theta + (int64_t)b * dtb : th;         // (never read without has_dth: a readable address for the loads in front of the select)
    double pc[WU ? Mdl::NPCU : Mdl::NPC];
    if constexpr (WU) Mdl::precompute_u(th, pc); else Mdl::precompute(th, pc);
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* ub = u + (int64_t)b * T * NU;
    const double* dub = WU ? d_u + (int64_t)b * T * NU : nullptr;
    double* ob = d_x + (int64_t)b * (T + 1) * NX;
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    // per-lane pool offsets (o) and row multipliers (m): row `lane` of F, w_t[lane]
    int fo[NX], fm[NX], wo = 0, wm = 0;
#pragma unroll
    for (int k = 0; k < NX; ++k) pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(0, lane * NX + k) : -1, fo[k], fm[k]);
    if (lane < NX) { wo = NC + GX + lane; wm = STRIDE; }
    double dx = (d_x0 && lane < NX) ? d_x0[(int64_t)b * NX + lane] : 0.0;  // dx_0
    if (lane < NX) ob[lane] = dx;
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = 0; c < nchunk; ++c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        wave_lds_sync();
        if (lane < cnt) {
            const int t = t0 + lane;
            double xc[NX], uc[NU], w[NX];
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) { xc[i] = xb[t * NX + i]; w[i] = 0.0; }
#pragma unroll
            for (int i = 0; i < NU; ++i) uc[i] = ub[t * NU + i];
            JvpPathSink<Mdl> s{row, w, dth, has_dth};
            Mdl::eval_path(xc, uc, nullptr, th, pc, s);
#pragma unroll
            for (int i = 0; i < NX; ++i) {                                 // the constant entries of E
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const int code = Mdl::path_code(1, i * NP + j);
                    if (code <= -2) w[i] += Mdl::path_const(-2 - code) * (has_dth ? dth[j] : 0.0);
                }
            }
            if constexpr (WU) {
                double duc[NU];
#pragma unroll
                for (int i = 0; i < NU; ++i) duc[i] = dub[t * NU + i];
                JvpPathuSink<Mdl> su{w, duc};
                Mdl::eval_pathu(xc, uc, nullptr, th, pc, su);
#pragma unroll
                for (int i = 0; i < NX; ++i) {                             // ... and of G
#pragma unroll
                    for (int j = 0; j < NU; ++j) {
                        const int code = Mdl::pathu_code(0, i * NU + j);
                        if (code <= -2) w[i] += Mdl::pathu_const(-2 - code) * duc[j];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) row[GX + i] = w[i];
        }
        wave_lds_sync();
        for (int tl = 0; tl < cnt; ++tl) {
            double x_new = blk[wo + tl * wm];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double xk = readlane_f64(dx, k);
                x_new += blk[fo[k] + tl * fm[k]] * xk;
            }
            dx = x_new;
            if (lane < NX) ob[(t0 + tl + 1) * NX + lane] = dx;
        }
    }
}

}  // namespace pdp
