// pdp_oc_x0_vjp_kernels.h - the gradient of a scalar loss L(x_0 .. x_T, u_0 .. u_{T-1}) of the OC solution with respect to the INITIAL STATE
// (pdp_oc_sens_out.grad_x0, include/pdp_hip.h), by an adjoint sweep behind the fused unit's launch.  For the auxiliary LQ system at (x, u, lam, theta) the initial state
// is n further parameters whose columns see E = 0, Hxe = Hue = hxe = 0 and X_0 = I: their feed-forward term k_t and their W_t vanish, so that with the Riccati gains K_t
// of the fused unit (u = -K x - k: the forward sweep's U = -K X - k)
//     du_t/dx_0 = -K_t Phi_t ,   Phi_{t+1} = (F_t - G_t K_t) Phi_t ,   Phi_0 = I
// and, with the cotangents gx_t = dL/dx_t, gu_t = dL/du_t,
//     mu_T = gx_T ;   t = T-1 .. 0 :   v_t = gu_t + G_t' mu_{t+1} ,   mu_t = gx_t + F_t' mu_{t+1} - K_t' v_t ;   dL/dx_0 = mu_0
// O(T (n^2 + n m)) and nothing larger than a vector per step.  Everything it reads lies in global memory once the fused launch has run: x, u, theta, the cotangents
// and K_t - the first NU x NX doubles (row-major) of a step's record in the gain workspace, fused_gain_doubles<Mdl>() doubles per step, which both fused kernels write.
// F_t, G_t are the models' `solf` group.  The fused kernels are not touched.  DESIGN.md section 4.1m.
#pragma once
#include "pdp_model_kernels.h"
#include "pdp_sweep_pool.h"

namespace pdp {

// A sweep kernel on OcX0VjpPool (pdp_sweep_pool.h: the block, the rows, the structure), on the trajectory and the gains the fused launch left behind.  The chunks are
// visited last to first.  Per chunk: lane tl loads x_t, u_t of step t = t0 + tl, evaluates the `solf` group through a PackedSink into pool row tl, copies K_t from
// the gain workspace behind it and puts the step's cotangents behind that - COT: gx_t, gu_t as the caller gave them (gx_0 included: it enters grad_x0 and nothing
// else); else the default mode's residuals x_t - demo_x_t, u_t - demo_u_t, which gives half the gradient of the demonstration loss, the convention of `grad`.  Then the serial sweep over the chunk's steps: lane i < NX owns mu[i] and reads column i of F_t
// and of K_t, lane NX + j (j < NU) owns v[j] and reads column j of G_t.  mu_{t+1}[k] reaches all of them as a scalar (v_readlane of its owner's register), then v_t[j]
// reaches the mu lanes the same way: two broadcast rounds per step, no LDS write / read pair and no global read on the recursion's chain - the pool reads of a step do
// not depend on mu.  The lanes behind NX + NU read blk[0] throughout.  No masking, no status word: a trajectory whose gains (or x, u, theta, cotangents) are not finite
// gets a non-finite row, and that row only.
template <class Mdl, bool COT>
__global__ void __launch_bounds__(64) oc_x0_vjp_kernel(int B, int T, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ theta, int tb,
                                                        const double* __restrict__ gx, const double* __restrict__ gu, const double* __restrict__ ws_gain,
                                                        double* __restrict__ grad_x0, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, GSZ = fused_gain_doubles<Mdl>();
    using Pool = OcX0VjpPool<Mdl>;
    constexpr int NC = Pool::NC, KO = Pool::KO, GXO = Pool::GXO, GUO = Pool::GUO, STRIDE = Pool::STRIDE;
    static_assert(NX + NU <= 64, "a lane per component of (mu, v)");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* blk = lds;
    double* pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* th = theta + (int64_t)b * tb;
    double pc[Mdl::NPC];
    Mdl::precompute(th, pc);
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* ub = u + (int64_t)b * T * NU;
    const double* gxb = gx + (int64_t)b * (T + 1) * NX;
    const double* gub = gu + (int64_t)b * T * NU;
    const double* gw = ws_gain + (int64_t)b * T * GSZ;
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::SOLF_NCONST; i_ += 64) blk[1 + i_] = Mdl::solf_const(i_);
    // per-lane pool offsets (o) and row multipliers (m): column `lane` of F / column lane - NX of G, this lane's cotangent, column `lane` of K
    const bool isx = lane < NX, isu = lane >= NX && lane < NX + NU;
    int ao[NX], am[NX], ko[NU], km[NU], go = 0, gm = 0;
#pragma unroll
    for (int k = 0; k < NX; ++k) pool_enc<NC, STRIDE>(isx ? Mdl::solf_code(0, k * NX + lane) : (isu ? Mdl::solf_code(1, k * NU + (lane - NX)) : -1), ao[k], am[k]);
#pragma unroll
    for (int j = 0; j < NU; ++j) { ko[j] = isx ? NC + KO + j * NX + lane : 0; km[j] = isx ? STRIDE : 0; }
    if (isx) { go = NC + GXO + lane; gm = STRIDE; }
    if (isu) { go = NC + GUO + (lane - NX); gm = STRIDE; }
    double mu = 0.0;                                                       // mu_T = gx_T
    if (isx) mu = COT ? gxb[(int64_t)T * NX + lane] : xb[(int64_t)T * NX + lane] - gxb[(int64_t)T * NX + lane];
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
            for (int i = 0; i < NX; ++i) { xc[i] = xb[t * NX + i]; row[GXO + i] = COT ? gxb[t * NX + i] : xc[i] - gxb[t * NX + i]; }
#pragma unroll
            for (int i = 0; i < NU; ++i) { uc[i] = ub[t * NU + i]; row[GUO + i] = COT ? gub[t * NU + i] : uc[i] - gub[t * NU + i]; }
#pragma unroll
            for (int i = 0; i < NX * NU; ++i) row[KO + i] = gw[(int64_t)t * GSZ + i];
            PackedSink s{row};
            Mdl::eval_solf(xc, uc, nullptr, th, pc, s);
        }
        wave_lds_sync();
        for (int tl = cnt - 1; tl >= 0; --tl) {
            double a = blk[go + tl * gm];                                  // lanes of mu: gx_t + F_t' mu_{t+1}; lanes of v: gu_t + G_t' mu_{t+1}
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double mk = readlane_f64(mu, k);
                a += blk[ao[k] + tl * am[k]] * mk;
            }
            double m_new = a;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                // (readlane_f64 spelled out, high half first: with the helper's order the v_fma below comes out with its two factors swapped - DESIGN.md section 4.1n)
                const double vj = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a), NX + j), __builtin_amdgcn_readlane(__double2loint(a), NX + j));
                m_new -= blk[ko[j] + tl * km[j]] * vj;
            }
            mu = m_new;
        }
    }
    if (isx) grad_x0[(int64_t)b * NX + lane] = mu;
}

}  // namespace pdp
