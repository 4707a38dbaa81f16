// pdp_sweep_pool.h - what the rollout sweep kernels share: sysid_vjp_kernel, sysid_vjp_u_kernel (pdp_sysid_vjp_kernels.h), sysid_jvp_kernel (pdp_sysid_jvp_kernels.h),
// oc_x0_vjp_kernel (pdp_oc_x0_vjp_kernels.h), cp_vjp_kernel (pdp_cp_vjp_kernels.h), cp_jvp_kernel (pdp_cp_jvp_kernels.h) and, for pool_enc alone, cp_step_adjoint_kernel (pdp_model_kernels.h).  One wavefront per trajectory on a given rollout;
// the horizon is cut into chunks of equal length <= rows; per chunk a lane-per-step pass packs the step's Jacobian entries into a pool row, then a serial sweep reads
// the rows through per-lane (offset, multiplier) pairs and broadcasts the carried vector with readlane_f64 (pdp_tile.h).  Shared here: the layout of the LDS block, the
// rule for its rows and the offset code.  Written out in every kernel, because a shared spelling did not keep their instructions: the chunk
// arithmetic and the fill of the constants.
#pragma once
#include "pdp_tile.h"

namespace pdp {

// The block, in doubles of dynamic LDS:
//     blk[0] = 0.0 | NCONST constants of the model's group(s) | rows x STRIDE: a row = NVAR packed variable entries | TAIL doubles of the kernel's own
// A Jacobian entry is read as blk[o + tl * m] for the row tl: a variable entry has o = NC + its slot, m = STRIDE; a structural zero reads blk[0] and a constant its
// slot behind it, both with m = 0 - no branch in the sweep.  STRIDE is made odd so that the 64 lanes of the lane-per-step pass, which write the same slot of 64
// adjacent rows, fall into different LDS banks.  slice(rows): the block rounded up to 16 bytes.
template <int NVAR, int NCONST, int TAIL>
struct SweepPool {
    static constexpr int NC = 1 + NCONST;
    static constexpr int STRIDE = (NVAR + TAIL) | 1;
    __host__ __device__ static constexpr int slice(int rows) { return (NC + rows * STRIDE + 1) & ~1; }
};
// sysid_vjp_kernel, sysid_jvp_kernel: the entries of (F_t, E_t) | GX: the NX cotangents g_t / the forcing term w_t
template <class Mdl>
struct SysidVjpPool : SweepPool<Mdl::PATH_NVAR, Mdl::PATH_NCONST, Mdl::NX> { static constexpr int GX = Mdl::PATH_NVAR; };
// sysid_vjp_u_kernel: the entries of (F_t, E_t), then those of G_t | GX: the NX cotangents | SU: NU doubles in which the sweep leaves this step's dL/du_t; the
// constants of both groups behind blk[0]
template <class Mdl>
struct SysidVjpUPool : SweepPool<Mdl::PATH_NVAR + Mdl::PATHU_NVAR, Mdl::PATH_NCONST + Mdl::PATHU_NCONST, Mdl::NX + Mdl::NU> {
    static constexpr int GX = Mdl::PATH_NVAR + Mdl::PATHU_NVAR, SU = GX + Mdl::NX;
};
// oc_x0_vjp_kernel: the entries of (F_t, G_t) | KO: K_t [NU][NX] | GXO: gx_t [NX] | GUO: gu_t [NU]
template <class Mdl>
struct OcX0VjpPool : SweepPool<Mdl::SOLF_NVAR, Mdl::SOLF_NCONST, Mdl::NX * Mdl::NU + Mdl::NX + Mdl::NU> {
    static constexpr int KO = Mdl::SOLF_NVAR, GXO = KO + Mdl::NX * Mdl::NU, GUO = GXO + Mdl::NX;
};
// cp_vjp_kernel: the entries of the `path` group (F_t, G_t; its c_x, c_u slots are written and never read) | GXO: gx_t [NX] | GUO: gu_t [NU] | XO: x_t [NX], from which
// an MLP policy's forward at step t reads its input | UO: u_t [NU] as the MLP's forward re-derived it, for the row's Jacobian pass.  A Lagrange policy has no use for
// the last two: in their place, from BO = XO, the values b_i(t) of its at most 16 basis functions, the second factor of its gradient slots.  Rows: oc_x0_vjp_rows_of.
template <class Mdl>
struct CpVjpPool : SweepPool<Mdl::PATH_NVAR, Mdl::PATH_NCONST, Mdl::NX + Mdl::NU + (Mdl::NX + Mdl::NU > 16 ? Mdl::NX + Mdl::NU : 16)> {
    static constexpr int GXO = Mdl::PATH_NVAR, GUO = GXO + Mdl::NX, XO = GUO + Mdl::NU, UO = XO + Mdl::NX, BO = XO;
};
// cp_jvp_kernel: the entries of the `path` group (as above) | XO: x_t [NX], the input of an MLP policy's pass at step t | DUO: du_t [NU] of a Lagrange policy, which
// does not depend on the recursion and is summed by the lane that evaluates the step (an MLP policy's du_t never reaches the row).  Rows: oc_x0_vjp_rows_of.
template <class Mdl>
struct CpJvpPool : SweepPool<Mdl::PATH_NVAR, Mdl::PATH_NCONST, Mdl::NX + Mdl::NU> {
    static constexpr int XO = Mdl::PATH_NVAR, DUO = XO + Mdl::NX;
};

// Pool rows (time steps per lane-parallel Jacobian pass).  A pool of at most SWEEP_POOL_DOUBLES (18.75 KB: with the constants and the allocation granularity an
// eighth of the CU's 160 KB) leaves two workgroups per SIMD resident, which fill each other's waits.  Both rules read the row stride alone, so Python restates them
// (runtime.ModelLib.sysid_vjp_rows, .oc_x0_vjp_rows, .cp_vjp_rows, .cp_jvp_rows).  The result bits do not depend on the rows: a sweep visits the steps in the same order whatever the pass they
// were evaluated in.
constexpr int SWEEP_POOL_DOUBLES = 2400;
// the SysID sweeps: the generated CHUNK while a CU holds at most one trajectory per SIMD; a larger batch what the pool holds, if that is at least 4 rows (the rule of
// sysid_rows).  With sysid_vjp_u_kernel's longer row a pool of CHUNK rows can exceed the LDS: the host's 150 KB bound sees that.
inline int sysid_vjp_rows_of(int B, int cus, int stride, int chunk) {
    if (B <= 4 * cus) return chunk;
    const int fit = SWEEP_POOL_DOUBLES / stride;
    return fit >= 4 ? (fit < chunk ? fit : chunk) : chunk;
}
// oc_x0_vjp_kernel, cp_vjp_kernel and cp_jvp_kernel, whatever the batch: what the pool holds, at least 4 and at most 64 (a lane per step)
constexpr int oc_x0_vjp_rows_of(int stride) { return SWEEP_POOL_DOUBLES / stride < 4 ? 4 : (SWEEP_POOL_DOUBLES / stride > 64 ? 64 : SWEEP_POOL_DOUBLES / stride); }

// the (offset, multiplier) pair of a group's code (Mdl::path_code and its like): >= 0 a variable slot, -1 a structural zero, -2 - i constant i
template <int NC, int STRIDE>
PDP_DEV void pool_enc(int code, int& o, int& m) { if (code >= 0) { o = NC + code; m = STRIDE; } else { o = (code == -1) ? 0 : 1 + (-2 - code); m = 0; } }

}  // namespace pdp
