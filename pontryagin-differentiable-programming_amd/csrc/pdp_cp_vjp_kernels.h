// pdp_cp_vjp_kernels.h - the gradient of a scalar loss L(x_0 .. x_T, u_0 .. u_{T-1}) of a ControlPlanning rollout under a parametrised policy u_t = pi(t, x_t, theta),
// with respect to theta and to the initial state, by an adjoint sweep on the given rollout (pdp_policy_cot behind PDP_POLICY_COTANGENT, include/pdp_hip.h).  With
// F_t, G_t the Jacobians of the dynamics at (x_t, u_t) and the cotangents gx_t = dL/dx_t, gu_t = dL/du_t
//     mu_T = gx_T ;   t = T-1 .. 0 :   v_t = gu_t + G_t' mu_{t+1} ,   dL/dtheta += (d pi/d theta)(t, x_t)' v_t ,   mu_t = gx_t + F_t' mu_{t+1} + (d pi/dx)(t, x_t)' v_t ;
//     dL/dx_0 = mu_0
// - the backward half of cp_step_adjoint_kernel (pdp_model_kernels.h) with the caller's cotangents where c_x, c_u, h_x stood: O(T (n^2 + n m + p)), nothing larger than a
// vector per step.  F_t, G_t are the models' `path` group; its c_x, c_u slots are written by eval_path and never read.  The step kernels are not touched.
// DESIGN.md section 4.1o.
#pragma once
#include "pdp_model_kernels.h"
#include "pdp_sweep_pool.h"

namespace pdp {

// Dynamic LDS of cp_vjp_kernel, in doubles: theta [p, made even] | zs: the layer inputs z_k of the current step, 8 x MLP_MAX_WIDTH, and a constant 1.0 for the biases |
// ds: the layer deltas of the current step, 8 x MLP_MAX_WIDTH | one double of padding | the block of CpVjpPool (pdp_sweep_pool.h)
struct CpVjpLayout { int zs, ds, blk, total; };
template <class Mdl>
__host__ __device__ inline CpVjpLayout cp_vjp_layout(int p, int rows) {
    CpVjpLayout L;
    L.zs = (p + 1) & ~1;
    L.ds = L.zs + 8 * MLP_MAX_WIDTH + 1;
    L.blk = L.ds + 8 * MLP_MAX_WIDTH + 1;
    L.total = L.blk + CpVjpPool<Mdl>::slice(rows);
    return L;
}

// A sweep kernel on CpVjpPool (pdp_sweep_pool.h: the block, the rows, the structure).  One wavefront per trajectory; theta in LDS; the chunks are visited last to
// first.  Per chunk: lane tl loads x_t, gx_t, gu_t of step t = t0 + tl into the tail of pool row tl (the only global reads inside the loop); u_t is re-derived - Lagrange:
// by the lane itself; MLP: by the whole wavefront, a step at a time, lanes = rows of a layer, from the x_t in the row (the forward of cp_step_adjoint_kernel's
// policy_forward) - then lane tl evaluates the `path` group through a PackedSink into its row.  Then the serial sweep over the chunk's steps: lane i < NX owns mu[i]
// in a register and reads column i of F_t, lane j < NU owns v[j] and reads column j of G_t; mu_{t+1}[k] reaches all of them as a scalar (v_readlane of its owner's
// register).  The hidden activations of step t are recomputed from the row's x_t into zs - nothing of the forward pass is stored - and the layer deltas go through ds
// as in cp_step_adjoint_kernel.  Each lane owns 8 gradient slots (parameter lane + 64 q), accumulated as there, in that kernel's order per slot and per mu component:
// with the cost's own gradients as cotangents the result is ControlPlanning.step's to rounding.  No masking: a trajectory whose inputs are not finite gets a
// non-finite row, and that row only.  grad or grad_x0 may be null.
template <class Mdl>
__global__ void __launch_bounds__(64) cp_vjp_kernel(int B, int T, pdp_policy pol, int p, const double* __restrict__ x, const double* __restrict__ theta, int tb,
                                                     const double* __restrict__ gx, const double* __restrict__ gu, double* __restrict__ grad,
                                                     double* __restrict__ grad_x0, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, W = MLP_MAX_WIDTH;
    using Pool = CpVjpPool<Mdl>;
    constexpr int NC = Pool::NC, STRIDE = Pool::STRIDE, GXO = Pool::GXO, GUO = Pool::GUO, XO = Pool::XO, UO = Pool::UO, BO = Pool::BO;
    static_assert(NX <= W && NX <= 64 && NU <= 64, "a lane per component of mu and of v; x_t is the input of a layer");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const CpVjpLayout L = cp_vjp_layout<Mdl>(p, CH);
    double *ths = lds, *zs = lds + L.zs, *ds = lds + L.ds, *blk = lds + L.blk, *pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool mlp = pol.kind == PDP_POLICY_MLP;
    const int nl = mlp ? pol.n_layers : 0, np = pol.n_pivots;
    double pc[Mdl::NPC];
    Mdl::precompute(nullptr, pc);
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* gxb = gx + (int64_t)b * (T + 1) * NX;
    const double* gub = gu + (int64_t)b * T * NU;
    for (int i = lane; i < p; i += 64) ths[i] = theta[(int64_t)b * tb + i];
    if (lane == 0) { blk[0] = 0.0; zs[8 * W] = 1.0; }
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    // per-lane parameter slots q = 0..7 (parameter index lane + 64 q): LDS offsets of the two factors of dL / d theta_j (as in cp_step_adjoint_kernel)
    int pr[8], pz[8], pzm[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int j = lane + 64 * q;
        pr[q] = L.ds; pz[q] = L.blk; pzm[q] = 0;       // blk[0] == 0.0 -> contributes nothing
        if (j < p) {
            if (mlp) {
                int off = 0, cols = NX;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k < nl) {
                        const int rows = pol.sizes[k], nw = rows * cols;
                        if (j >= off && j < off + nw + rows) {
                            const int e = j - off;
                            if (e < nw) { pr[q] = L.ds + k * W + e % rows; pz[q] = L.zs + k * W + e / rows; }     // vec_F(A_k): row + col*rows
                            else { pr[q] = L.ds + k * W + (e - nw); pz[q] = L.zs + 8 * W; }                     // bias: factor 1.0
                        }
                        off += nw + rows; cols = rows;
                    }
                }
            } else { pr[q] = L.ds + j % NU; pz[q] = L.blk + NC + BO + j / NU; pzm[q] = STRIDE; }       // theta = vcat(U_0..U_N): delta = v[j % m], factor = b_{j / m}(t) of the row
        }
    }
    double gacc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) gacc[q] = 0.0;
    // per-lane pool offsets (o) and row multipliers (m): column `lane` of F (lane < NX) and of G (lane < NU), this lane's cotangents
    int fo[NX], fm[NX], go[NX], gm[NX];
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(0, k * NX + lane) : -1, fo[k], fm[k]);
        pool_enc<NC, STRIDE>(lane < NU ? Mdl::path_code(1, k * NU + lane) : -1, go[k], gm[k]);
    }
    const int gxo = lane < NX ? NC + GXO + lane : 0, gxm = lane < NX ? STRIDE : 0;
    const int guo = lane < NU ? NC + GUO + lane : 0, gum = lane < NU ? STRIDE : 0;
    double mu = 0.0;                                                       // mu_T = gx_T
    if (lane < NX) mu = gxb[(int64_t)T * NX + lane];
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = nchunk - 1; c >= 0; --c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        wave_lds_sync();
        if (lane < cnt) {
            const int t = t0 + lane;
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) { row[XO + i] = xb[t * NX + i]; row[GXO + i] = gxb[t * NX + i]; }
#pragma unroll
            for (int i = 0; i < NU; ++i) row[GUO + i] = gub[t * NU + i];
        }
        wave_lds_sync();
        if (mlp) {
            // u_t of the chunk's steps, the wavefront on one step at a time: a = b_k + A_k z_k, lanes = rows
            for (int tl = 0; tl < cnt; ++tl) {
                double* row = pool + tl * STRIDE;
                if (lane < NX) zs[lane] = row[XO + lane];
                wave_lds_sync();
                int off = 0, cols = NX;
                for (int k = 0; k < nl; ++k) {
                    const int rows = pol.sizes[k];
                    double a = 0.0;
                    if (lane < rows) {
                        a = ths[off + rows * cols + lane];
#pragma unroll 4
                        for (int cc = 0; cc < cols; ++cc) a += ths[off + lane + cc * rows] * zs[k * W + cc];
                    }
                    if (k + 1 < nl) {
                        const double zk = pdp_tanh(a);
                        if (lane < rows) zs[(k + 1) * W + lane] = zk;
                    } else if (lane < NU) row[UO + lane] = a;
                    wave_lds_sync();
                    off += rows * cols + rows; cols = rows;
                }
            }
        }
        if (lane < cnt) {
            const int t = t0 + lane;
            double xc[NX], uc[NU];
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) xc[i] = row[XO + i];
            if (!mlp) {                                                    // the basis values of the step stay in the row for the sweep
#pragma unroll
                for (int j = 0; j < NU; ++j) uc[j] = 0.0;
                for (int i = 0; i < np; ++i) {
                    const double bi = lagrange_basis(pol, i, (double)t);
                    row[BO + i] = bi;
#pragma unroll
                    for (int j = 0; j < NU; ++j) uc[j] += bi * ths[i * NU + j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < NU; ++j) uc[j] = row[UO + j];
            }
            PackedSink sk{row};
            Mdl::eval_path(xc, uc, nullptr, nullptr, pc, sk);
        }
        wave_lds_sync();
        for (int tl = cnt - 1; tl >= 0; --tl) {
            // v = gu + G' mu
            double v = blk[guo + tl * gum];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double mk = readlane_f64(mu, k);
                v += blk[go[k] + tl * gm[k]] * mk;
            }
            // the policy's backward pass: deltas per layer into ds, layer inputs into zs; dpx = (d pi/dx)' v on the lanes of mu
            double dpx = 0.0;
            if (!mlp) {
                if (lane < NU) ds[lane] = v;
                wave_lds_sync();
            } else {
                if (lane < NX) zs[lane] = blk[NC + XO + lane + tl * STRIDE];
                if (lane < NU) ds[(nl - 1) * W + lane] = v;
                wave_lds_sync();
                int off = 0, cols = NX;
                for (int k = 0; k + 1 < nl; ++k) {                         // the hidden activations of step t, recomputed
                    const int rows = pol.sizes[k];
                    double a = 0.0;
                    if (lane < rows) {
                        a = ths[off + rows * cols + lane];
#pragma unroll 4
                        for (int cc = 0; cc < cols; ++cc) a += ths[off + lane + cc * rows] * zs[k * W + cc];
                    }
                    const double zk = pdp_tanh(a);
                    if (lane < rows) zs[(k + 1) * W + lane] = zk;
                    wave_lds_sync();
                    off += rows * cols + rows; cols = rows;
                }
                for (int k = nl - 1; k >= 0; --k) {                        // off, cols: those of layer k
                    const int rows = pol.sizes[k];
                    double a = 0.0;
                    if (lane < cols) {
#pragma unroll 4
                        for (int r = 0; r < rows; ++r) a += ths[off + r + lane * rows] * ds[k * W + r];      // A_k' delta_k
                    }
                    if (k > 0) {
                        if (lane < cols) { const double zk = zs[k * W + lane]; ds[(k - 1) * W + lane] = a * (1.0 - zk * zk); }
                        const int prows = cols, pcols = k > 1 ? pol.sizes[k - 2] : NX;
                        off -= prows * pcols + prows; cols = pcols;
                    } else dpx = a;                                        // (zero behind lane NX: cols = NX)
                    wave_lds_sync();
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) gacc[q] += lds[pr[q]] * lds[pz[q] + tl * pzm[q]];
            // mu_t = gx + (d pi/dx)' v + F' mu
            double m_new = blk[gxo + tl * gxm] + dpx;
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const double mk = readlane_f64(mu, k);
                m_new += blk[fo[k] + tl * fm[k]] * mk;
            }
            mu = m_new;
            wave_lds_sync();
        }
    }
    if (grad) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { const int j = lane + 64 * q; if (j < p) grad[(int64_t)b * p + j] = gacc[q]; }
    }
    if (grad_x0 && lane < NX) grad_x0[(int64_t)b * NX + lane] = mu;
}

}  // namespace pdp
