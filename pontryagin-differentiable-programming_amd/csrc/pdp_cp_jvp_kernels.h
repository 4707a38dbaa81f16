// pdp_cp_jvp_kernels.h - the tangent of a ControlPlanning rollout under a parametrised policy u_t = pi(t, x_t, theta), x_{t+1} = f(x_t, u_t), along a direction
// (d_theta, d_x0), by a forward (tangent) sweep on the given rollout (pdp_policy_tan behind PDP_POLICY_TANGENT, include/pdp_hip.h).  With F_t, G_t the Jacobians of
// the dynamics at (x_t, u_t)
//     dx_0 given ;   t = 0 .. T-1 :   du_t = (d pi/dx)(t, x_t) dx_t + (d pi/d theta)(t, x_t) d_theta ,   dx_{t+1} = F_t dx_t + G_t du_t
// - one column of the forward sensitivities U_t = pi_x X_t + pi_theta, X_{t+1} = F_t X_t + G_t U_t (PDP.py:813-838): O(T (n^2 + n m + p)), nothing larger than a vector
// per step.  The other half of cp_vjp_kernel (pdp_cp_vjp_kernels.h): with both a Gauss-Newton product J' J v of any residual of the rollout is two launches whatever
// p is.  F_t, G_t are the models' `path` group; its c_x, c_u slots are written by eval_path and never read.  Instantiated for PDP_KIND_CP only (pdp_model.hip).
// DESIGN.md section 4.1p.
#pragma once
#include "pdp_model_kernels.h"
#include "pdp_sweep_pool.h"

namespace pdp {

// Dynamic LDS of cp_jvp_kernel, in doubles: theta [p, made even] | d_theta [p, made even] | zs: the layer inputs z_k of the current step, 8 x MLP_MAX_WIDTH |
// dzs: their tangents dz_k, 8 x MLP_MAX_WIDTH | the block of CpJvpPool (pdp_sweep_pool.h)
struct CpJvpLayout { int dth, zs, dzs, blk, total; };
template <class Mdl>
__host__ __device__ inline CpJvpLayout cp_jvp_layout(int p, int rows) {
    CpJvpLayout L;
    L.dth = (p + 1) & ~1;
    L.zs = 2 * L.dth;
    L.dzs = L.zs + 8 * MLP_MAX_WIDTH;
    L.blk = L.dzs + 8 * MLP_MAX_WIDTH;
    L.total = L.blk + CpJvpPool<Mdl>::slice(rows);
    return L;
}

// A sweep kernel on CpJvpPool (pdp_sweep_pool.h: the block, the rows, the structure): cp_vjp_kernel's rollout run forwards, structured like sysid_jvp_kernel.  One
// wavefront per trajectory; theta and d_theta in LDS (a NULL d_theta: +0.0); the chunks are visited first to last.  Per chunk lane tl loads x_t, u_t of step
// t = t0 + tl - the controls are GIVEN, nothing re-derives them - and evaluates the `path` group through a PackedSink into pool row tl; x_t stays in the row, where an MLP
// policy's pass reads its input.  Lagrange policy: d pi/dx = 0 and du_t[j] = sum_i b_i(t) d_theta[i m + j] does not depend on the recursion - the same lane sums it
// there and then, leaves it in the row and stores it to d_u; the serial loop evaluates no basis function.  Then the serial sweep over the chunk's steps: lane i < NX
// owns dx[i] in a register and reads ROW i of F_t and ROW i of G_t through (offset, multiplier) pairs formed once; dx_t[k] reaches every lane as a scalar (v_readlane
// of its owner's register).  MLP policy: one pass per layer, lanes = rows of the layer, computes the layer's value and its tangent together,
//     a = b_k + A_k z_k ,   da = db_k + dA_k z_k + A_k dz_k ;   z_{k+1} = tanh(a) ,   dz_{k+1} = (1 - z_{k+1}^2) da ;   the last layer is linear: du_t = da
// with z_0 = x_t read from the row and dz_0 = dx_t from the scalars; z_k, dz_k of the hidden layers go through zs, dzs; du_t[j] reaches the sweep by v_readlane of lane
// j.  Sums run in ascending index order.  Each step's dx_{t+1} (and the network's du_t) is stored directly to global memory; nothing waits for those stores.  No masking:
// a non-finite input reaches its own trajectory only.  d_x0 NULL: +0.0.  d_u may be NULL.
template <class Mdl>
__global__ void __launch_bounds__(64) cp_jvp_kernel(int B, int T, pdp_policy pol, int p, const double* __restrict__ x, const double* __restrict__ u,
                                                     const double* __restrict__ theta, int tb, const double* __restrict__ d_theta, int dtb,
                                                     const double* __restrict__ d_x0, double* __restrict__ d_x, double* __restrict__ d_u, int CH) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, W = MLP_MAX_WIDTH;
    using Pool = CpJvpPool<Mdl>;
    constexpr int NC = Pool::NC, STRIDE = Pool::STRIDE, XO = Pool::XO, DUO = Pool::DUO;
    static_assert(NX <= W && NX <= 64 && NU <= 64, "a lane per component of dx and of du; x_t is the input of a layer");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const CpJvpLayout L = cp_jvp_layout<Mdl>(p, CH);
    double *ths = lds, *dths = lds + L.dth, *zs = lds + L.zs, *dzs = lds + L.dzs, *blk = lds + L.blk, *pool = blk + NC;
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool mlp = pol.kind == PDP_POLICY_MLP;
    const int nl = mlp ? pol.n_layers : 0, np = pol.n_pivots;
    double pc[Mdl::NPC];
    Mdl::precompute(nullptr, pc);
    const double* xb = x + (int64_t)b * (T + 1) * NX;
    const double* ub = u + (int64_t)b * T * NU;
    double* ob = d_x + (int64_t)b * (T + 1) * NX;
    double* oub = d_u ? d_u + (int64_t)b * T * NU : nullptr;
    for (int i = lane; i < p; i += 64) {
        ths[i] = theta[(int64_t)b * tb + i];
        dths[i] = d_theta ? d_theta[(int64_t)b * dtb + i] : 0.0;
    }
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    // per-lane pool offsets (o) and row multipliers (m): row `lane` of F and of G
    int fo[NX], fm[NX], go[NU], gm[NU];
#pragma unroll
    for (int k = 0; k < NX; ++k) pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(0, lane * NX + k) : -1, fo[k], fm[k]);
#pragma unroll
    for (int j = 0; j < NU; ++j) pool_enc<NC, STRIDE>(lane < NX ? Mdl::path_code(1, lane * NU + j) : -1, go[j], gm[j]);
    double dx = (d_x0 && lane < NX) ? d_x0[(int64_t)b * NX + lane] : 0.0;  // dx_0
    if (lane < NX) ob[lane] = dx;
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = 0; c < nchunk; ++c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        wave_lds_sync();
        if (lane < cnt) {
            const int t = t0 + lane;
            double xc[NX], uc[NU];
            double* row = pool + lane * STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) { xc[i] = xb[t * NX + i]; row[XO + i] = xc[i]; }
#pragma unroll
            for (int j = 0; j < NU; ++j) uc[j] = ub[t * NU + j];
            if (!mlp) {                                                    // du_t = (d pi/d theta)(t) d_theta: it stays in the row for the sweep
                double du[NU];
#pragma unroll
                for (int j = 0; j < NU; ++j) du[j] = 0.0;
                for (int i = 0; i < np; ++i) {
                    const double bi = lagrange_basis(pol, i, (double)t);
#pragma unroll
                    for (int j = 0; j < NU; ++j) du[j] += bi * dths[i * NU + j];
                }
#pragma unroll
                for (int j = 0; j < NU; ++j) { row[DUO + j] = du[j]; if (oub) oub[t * NU + j] = du[j]; }
            }
            PackedSink sk{row};
            Mdl::eval_path(xc, uc, nullptr, nullptr, pc, sk);
        }
        wave_lds_sync();
        for (int tl = 0; tl < cnt; ++tl) {
            double xk[NX], duj[NU];
#pragma unroll
            for (int k = 0; k < NX; ++k) xk[k] = readlane_f64(dx, k);
            if (!mlp) {
#pragma unroll
                for (int j = 0; j < NU; ++j) duj[j] = blk[NC + DUO + j + tl * STRIDE];
            } else {
                // the policy's pass: value and tangent of a layer together, lanes = rows
                const double* xr = blk + NC + XO + tl * STRIDE;
                double da = 0.0;
                int off = 0, cols = NX;
                for (int k = 0; k < nl; ++k) {
                    const int rows = pol.sizes[k];
                    double a = 0.0, d = 0.0;
                    if (lane < rows) {
                        a = ths[off + rows * cols + lane];
                        d = dths[off + rows * cols + lane];
                        if (k == 0) {                                      // z_0 = x_t from the row, dz_0 = dx_t from the scalars
#pragma unroll 4
                            for (int cc = 0; cc < NX; ++cc) {
                                const double A = ths[lane + cc * rows], z = xr[cc];
                                a += A * z;
                                d += dths[lane + cc * rows] * z + A * xk[cc];
                            }
                        } else {
#pragma unroll 4
                            for (int cc = 0; cc < cols; ++cc) {
                                const double A = ths[off + lane + cc * rows], z = zs[k * W + cc];
                                a += A * z;
                                d += dths[off + lane + cc * rows] * z + A * dzs[k * W + cc];
                            }
                        }
                    }
                    if (k + 1 < nl) {
                        const double zk = pdp_tanh(a);
                        if (lane < rows) { zs[(k + 1) * W + lane] = zk; dzs[(k + 1) * W + lane] = (1.0 - zk * zk) * d; }
                        wave_lds_sync();
                    } else da = d;
                    off += rows * cols + rows; cols = rows;
                }
                if (oub && lane < NU) oub[(t0 + tl) * NU + lane] = da;
#pragma unroll
                for (int j = 0; j < NU; ++j) duj[j] = readlane_f64(da, j);
            }
            // dx_{t+1} = F dx + G du
            double x_new = 0.0;
#pragma unroll
            for (int k = 0; k < NX; ++k) x_new += blk[fo[k] + tl * fm[k]] * xk[k];
#pragma unroll
            for (int j = 0; j < NU; ++j) x_new += blk[go[j] + tl * gm[j]] * duj[j];
            dx = x_new;
            if (lane < NX) ob[(t0 + tl + 1) * NX + lane] = dx;
        }
    }
}

}  // namespace pdp
