// pdp_chain_rule.h - the chain rule of the sum-of-squares loss through the sensitivity tiles of a forward sweep, once, for the four fused units:
// oc_pdp_fused_kernel (pdp_model_kernels.h), oc_pdp_fused3_kernel (pdp_fused3_kernels.h), sysid_step_kernel and sysid_step2_kernel (both in
// pdp_sysid_step_kernels.h).  With the residuals d_t = x_t - x_demo,t (OC: also u_t - u_demo,t) and the sensitivities X_t = dx_t/dtheta, U_t = du_t/dtheta:
//     loss = sum_t |d_t|^2      grad = sum_t d_t' X_t (+ d_t' U_t)      G = sum_t X_t' X_t (+ U_t' U_t)   (Gauss-Newton, J'J)
// A unit's lane-per-step pass leaves d_t in the DLX / DLU slots of its LDS pool row (residual_slot); its sensitivity loop gathers them as the tiles DX, DU - the
// residual of a row broadcast over its columns, element-aligned with X_t, U_t - and contracts step by step (contract_step); the stage T, which no pool row
// holds, goes through the dlT staging and the same mask (observed).  Everything is forced inline, and NO ADDRESS
// IS FORMED INSIDE A HELPER (no pointer parameter is indexed; a reference names one element the caller chose): an address formed in a helper is simplified on its
// own before the helper is inlined and then no longer folds with the kernel's other addresses as its own text did.  That is why the terminal row's loop over
// dlT[row] stays in the kernels - as terminal_row(dlT, ...) it changed the LDS addressing, and with it the instructions, of the frozen instantiations, which
// are to compile to what they compiled to with the text in place (profiles/chain_rule_code_object_diff.txt).  The two SysID kernels stand side by side in
// pdp_sysid_step_kernels.h behind what they share (layout, argument pack, rollout); its header says which parts of the step stayed in their text, by the same rule.
//
// The modes - a template parameter of the kernels, never a run-time branch; an instantiation contains only its own arms:
//   PDP_FUSED_PLAIN  loss and gradient of the demonstration loss (the frozen default);
//   PDP_FUSED_RIC    the same with the Riccati / prediction records (and, fused3, every sensitivity output) written;
//   PDP_FUSED_COT    PDP_OC_COTANGENT: demo_x / demo_u carry the cotangents gx = dL/dx [B][T+1][n], gu = dL/du [B][T][m] of a caller's scalar loss L(x, u) and go
//                    into the slots as they are, so that grad = sum_t gx_t' X_t + gu_t' U_t is the vector-Jacobian product of L through the OC solution,
//                    contracted in the same order into the same accumulators.  No loss is formed (`loss` may be NULL); gx[b][0] is never loaded (X_0 = 0).
//   PDP_FUSED_GN     PDP_GRAD_GAUSS_NEWTON: PDP_FUSED_PLAIN plus one accumulator tile Gn += X_t' X_t + U_t' U_t (the tiles are in registers anyway).  Both MFMA
//                    operands are the same tile: G[i][j] and G[j][i] are the same products in the same order, symmetric to the bit.  grad is then ONE PACKED ROW
//                    per trajectory, [B][p + 1 + p p] = gradient | loss | G row-major.  OC tiles carry the parameter block in rows and columns M .. M + p - 1.
//   PDP_FUSED_MISS, PDP_FUSED_GN_MISS   PDP_GRAD_SKIP_MISSING on PDP_FUSED_PLAIN / PDP_FUSED_GN: a NaN in demo_x / demo_u is an entry that was not observed.  No
//                    change of the LDS layout: the NaN left in the slot in place of the residual IS the mark (nothing is added to the loss for it), and the
//                    sensitivity loop SELECTS 0.0 for the residual and for the row of X_t / U_t wherever the residual tile is NaN (a compare and a select per tile
//                    register; never a product with 0: 0 inf must not appear) before it contracts.  Both operands of every G product carry the same row mask.
//                    The recursion itself and tile_finite keep looking at the unmasked sensitivities.
//   PDP_SYSID_PLAIN  loss and gradient of SysID.step (no control part; NT parameter tiles of 16 columns, parameters at column 0);
//   PDP_SYSID_GN     as PDP_FUSED_GN (G = sum_{t<=T} X_t' X_t); the rollout starts from the trailing argument x0 [B][NX] (NULL: x_obs[:, 0]), and row 0 adds
//                    |x0 - x_obs_0|^2 to the loss and - X_0 = 0 - nothing to gradient and G;
//   PDP_SYSID_GN_MISS   PDP_SYSID_GN with the semantics of PDP_GRAD_SKIP_MISSING.  An OBSERVED entry whose own state is not finite leaves a NaN in the loss: a
//                    diverged rollout stays visible (there is no status word here).
//                    Both SysID Gauss-Newton modes exist for one parameter tile only (NT == 1, p <= 16: what irl.lm_step solves on the host).
//   PDP_SYSID_GN_INI, PDP_SYSID_GN_INI_MISS   PDP_SYSID_GN / PDP_SYSID_GN_MISS with q = popcount(ini_mask) components of x0 as further unknowns (the second
//                    trailing argument: a bit mask over the n state components; its k-th set bit i_k, ascending, is unknown p + k).  dx_t/dx0[i_k] is one more
//                    COLUMN of the same sensitivity tile: it starts as the unit vector e_{i_k} instead of 0 (sysid_ini_tile, per lane, no LDS) and sees a zero column of
//                    E, which the E gather returns for every column >= p anyway - the recursion, the contraction and the Gram product are the ones of the other modes,
//                    no MFMA and no LDS word more per step.  W = p + q <= 16 (the host checks); the row is grad [W] | loss | G [W][W].  Row 0 is no longer silent: an
//                    observed x_obs[0][i_k] adds d_0[i_k] to grad[p + k] and 1 to G[p + k][p + k].
//   PDP_SYSID_GN_W, PDP_SYSID_GN_W_INI   weighted and Huber-robust least squares on PDP_SYSID_GN / PDP_SYSID_GN_INI (include/pdp_hip_sysid_wls.h).  The last trailing
//                    argument is a SysidWls: the weights, their batch stride, Huber's delta and whether PDP_GRAD_SKIP_MISSING holds - run-time values, uniform over the
//                    launch, NOT further template parameters.  An entry is observed iff w > 0 and (under the flag) x_obs is not NaN.  The lane-per-step pass leaves
//                    s d in the DLX slot and s = sqrt(w psi) in a SECOND group of NX slots of the same pool row (both 0.0 where the entry is not observed, by a select)
//                    and adds rho(e) to the loss (wls_slot: the division and the two square roots happen there, once per entry, lane-parallel); the sensitivity loop
//                    gathers the tile S beside DX and scales the rows of X_t by a guarded product (wls_scale: S != 0 ? S X : 0.0 - 0 inf cannot appear) before it
//                    contracts.  Both operands of every G product are the same scaled tile.  The recursion itself is never scaled.  The pool row is NX words longer.
//   PDP_FUSED_GN_W   the same on the two OC units (include/pdp_hip_oc_wls.h): always Gauss-Newton, weights on states AND controls.  The kernels' trailing pack holds one
//                    OcWls - the OC twin of SysidWls, split into one SysidWls per side (oc_wls_x, oc_wls_u) for wls_slot.  The lane-per-step pass leaves s d in the
//                    DLX / DLU slots and s in a SECOND group of NX + NU slots of the same forward pool row; the sensitivity loop gathers the tiles SX, SU beside DX, DU,
//                    forms Xm = wls_scale(SX, X_t), Um = wls_scale(SU, U_t) (register 0) and then does what the MISS arm does with them.  The terminal row goes through
//                    dlT, followed by NX more words for its s.  The forward row is NX + NU words longer and dlT NX words - in this mode only (the extra-words argument
//                    of the layouts); the Riccati recursion, the forward sweep and tile_finite see the unscaled tiles.
#pragma once
#include "pdp_tile.h"

#define PDP_FUSED_PLAIN 0
#define PDP_FUSED_RIC 1
#define PDP_FUSED_COT 2
#define PDP_FUSED_GN 3
#define PDP_FUSED_MISS 4
#define PDP_FUSED_GN_MISS 5
#define PDP_FUSED_GN_W 6

#define PDP_SYSID_PLAIN 0
#define PDP_SYSID_GN 1
#define PDP_SYSID_GN_MISS 2
#define PDP_SYSID_GN_INI 3
#define PDP_SYSID_GN_INI_MISS 4
#define PDP_SYSID_GN_W 5
#define PDP_SYSID_GN_W_INI 6

namespace pdp {

// what the residual slot holds and what it adds to the loss.  The two MISS rules differ only in WHICH NaN marks an entry that was not observed: the
// demonstration's own (OC units) or the difference's (SysID units); nothing but the select (observed) ever reads it.
enum Residual { RES_PLAIN, RES_MISS, RES_MISS_DIFF };

template <int MODE>
struct FusedMode {
    static_assert(MODE == PDP_FUSED_PLAIN || MODE == PDP_FUSED_RIC || MODE == PDP_FUSED_COT || MODE == PDP_FUSED_GN || MODE == PDP_FUSED_MISS || MODE == PDP_FUSED_GN_MISS ||
                      MODE == PDP_FUSED_GN_W,
                  "instantiation");
    static constexpr bool RIC = MODE == PDP_FUSED_RIC, COT = MODE == PDP_FUSED_COT, WLS = MODE == PDP_FUSED_GN_W;      // (WLS: its own observed-rule, never together with MISS)
    static constexpr bool GN = MODE == PDP_FUSED_GN || MODE == PDP_FUSED_GN_MISS || WLS;
    static constexpr bool MISS = MODE == PDP_FUSED_MISS || MODE == PDP_FUSED_GN_MISS;
    static constexpr Residual RES = MISS ? RES_MISS : RES_PLAIN;          // (COT forms no residual: the cotangent takes the slot as it is)
};
template <int MODE, int NT>                                // NT parameter tiles.  The kernels' trailing pack follows from MODE: SysidArgs<MODE> (pdp_sysid_step_kernels.h)
struct SysidMode {
    static constexpr bool WLS = MODE == PDP_SYSID_GN_W || MODE == PDP_SYSID_GN_W_INI;             // (its own observed-rule: never together with MISS)
    static constexpr bool INI = MODE == PDP_SYSID_GN_INI || MODE == PDP_SYSID_GN_INI_MISS || MODE == PDP_SYSID_GN_W_INI;
    static_assert(MODE == PDP_SYSID_PLAIN || (NT == 1 && MODE >= PDP_SYSID_GN && MODE <= PDP_SYSID_GN_W_INI), "instantiation");
    static constexpr bool GN = MODE != PDP_SYSID_PLAIN, MISS = MODE == PDP_SYSID_GN_MISS || MODE == PDP_SYSID_GN_INI_MISS;
    static constexpr Residual RES = MISS ? RES_MISS_DIFF : RES_PLAIN;
};

// ---- the residual-slot rule.  v: the state / control entry; dd: the demonstration's entry.  residual_value is what goes into
// the slot, residual_square its share of the loss (a missing entry: none).  residual_slot does both for one entry, the store between them as the kernels
// always had it; `slot` is the caller's LDS element - no address is formed in here.
template <Residual RES>
PDP_DEV double residual_value(double v, double dd) {
    if constexpr (RES == RES_MISS) { const double d = v - dd; return dd == dd ? d : dd; }
    else return v - dd;
}
template <Residual RES>
PDP_DEV double residual_square(double d, double dd) {
    if constexpr (RES == RES_PLAIN) return d * d;
    else return dd == dd ? d * d : 0.0;
}
template <Residual RES>
PDP_DEV void residual_slot(double& slot, double v, double dd, double& lsum) {
    const double d = residual_value<RES>(v, dd);
    slot = d;
    lsum += residual_square<RES>(d, dd);
}

// ---- the select-don't-multiply mask: v where the residual d of its row was observed; MISS: 0.0 where d is NaN (never a product with 0: 0 inf must not appear)
template <bool MISS>
PDP_DEV double observed(double d, double v) {
    if constexpr (MISS) return d == d ? v : 0.0;
    else return v;
}

// ---- Gn + X' X: both MFMA operands are the same tile.  SMALL (n <= 4): X lives on register 0 of its tile
template <bool SMALL>
PDP_DEV d4 gram_add(const d4 X, d4 Gn) {
    if constexpr (SMALL) return mma_tn_r0(X, X, Gn);
    else return mma_tn(X, X, Gn);
}

// ---- one step of the sensitivity loop.  DX, DU: the residual tiles of the step; X, U: its sensitivity tiles.  NR: the registers of DX that carry residuals
// (n <= 4: 1); U (m <= 4 rows) lives on register 0.  mask_step, once per step of the OC units: with MISS the residuals and the sensitivity rows selected to 0 where
// the residual is NaN (the selects are spelled on the tile elements, not through observed(): the form the kernels compiled from).  The SysID units have no control
// part - contract_step without DU, U and gram_add, not a zero tile that would cost an MFMA - and keep the three lines of their MISS arm in their own text
// (pdp_sysid_step_kernels.h): through mask_step their skip-missing instantiations gained or lost one to three instructions
// (profiles/chain_rule_code_object_diff.txt).
template <bool MISS, int NR>
PDP_DEV void mask_step(d4& DX, d4& DU, const d4 X, const d4 U, d4& Xm, d4& Um) {      // Xm, Um: X, U with MISS' mask
    if constexpr (MISS) {
        Xm = zero4(); Um = zero4();
#pragma unroll
        for (int r = 0; r < NR; ++r) { const bool obs = DX[r] == DX[r]; Xm[r] = obs ? X[r] : 0.0; DX[r] = obs ? DX[r] : 0.0; }
        { const bool obs = DU[0] == DU[0]; Um[0] = obs ? U[0] : 0.0; DU[0] = obs ? DU[0] : 0.0; }
    } else { Xm = X; Um = U; }
}
// Gn + X' X + U' U (without U: gram_add).  Called under `if constexpr (GN)`: an instantiation without G must not name its Gn tile inside the step's lambda (the
// capture alone changes the code of the frozen instantiations)
template <bool SMALL>
PDP_DEV d4 gram_step(const d4 X, const d4 U, d4 Gn) { return mma_tn_r0(U, U, gram_add<SMALL>(X, Gn)); }
// this lane's share of the gradient: DX . X (+ DU . U, the same left-to-right sum)
PDP_DEV double contract_step(const d4 DX, const d4 X) { return DX[0] * X[0] + DX[1] * X[1] + DX[2] * X[2] + DX[3] * X[3]; }
PDP_DEV double contract_step(const d4 DX, const d4 DU, const d4 X, const d4 U) { return contract_step(DX, X) + DU[0] * U[0]; }


// ---- PDP_SYSID_GN_INI*: the initial sensitivity tile X_0 [n][W] = zeros with X_0[i_k][p + k] = 1, and the width W = p + q of the row.  Per lane: its column minus p
// selects the k-th set bit of the mask (a scan over the NX bits, unrolled), its four rows are compared with it.  No memory is touched.
template <int NX, int NP>
PDP_DEV d4 sysid_ini_tile(int lane, unsigned mask) {
    const int k = tile_col(lane) - NP;
    int ik = -1, seen = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const bool set = (mask >> i) & 1u;
        ik = (set && seen == k) ? i : ik;
        seen += set ? 1 : 0;
    }
    d4 X;
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] = tile_row(lane, r) == ik ? 1.0 : 0.0;
    return X;
}
template <int NP>
PDP_DEV int sysid_ini_width(unsigned mask) { return NP + __builtin_popcount(mask); }
// G [W][W] row-major from the accumulator tile: store_dense with a RUN-TIME width, in a helper of its own.  store_dense itself must keep being called with
// compile-time R, C, ld only: the constants are propagated into it before it is inlined, and one caller with a run-time width changed the instructions of the frozen
// Gauss-Newton instantiations that call it with NP (profiles/sysid_ini_code_object_diff.txt).  Used by the PDP_SYSID_GN_INI* arms alone.
PDP_DEV void sysid_ini_store(double* __restrict__ G, int W, int lane, const d4 Gn) {
    const int col = tile_col(lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = tile_row(lane, r);
        if (row < W && col < W) G[row * W + col] = Gn[r];
    }
}


// ---- PDP_SYSID_GN_W*: weighted / Huber least squares.  The run-time arguments of the two modes, one struct at the end of the kernels' trailing pack.  `w` is never
// NULL: without weights the host passes x_obs (a readable block of the same shape) and has_w = 0, and the pass SELECTS 1.0 - no conditional block around the load.
struct SysidWls {
    const double* w;            // [B or 1][T+1][NX]
    long long bstride;          // (T+1) NX, or 0: one block shared by the batch
    double delta;               // Huber's threshold on the standardised residual; +inf: off
    int has_w, skip;            // weights given; PDP_GRAD_SKIP_MISSING
};
// the slot rule of one entry.  v: the state; o: x_obs; wl: the word loaded through SysidWls::w.  slot_d, slot_s: the caller's two LDS elements (no address is formed
// in here).  e = sqrt(w) d, psi = 1 (|e| <= delta) or delta / |e|, s = sqrt(w psi); rho = e^2 or 2 delta |e| - delta^2.  A NaN e takes the second branch of both and
// stays a NaN; delta = +inf takes the first for every finite and infinite e.
PDP_DEV void wls_slot(double& slot_d, double& slot_s, double v, double o, double wl, const SysidWls a, double& lsum) {
    const double w = a.has_w ? wl : 1.0;
    const double d = v - o;
    const bool obs = (w > 0.0) && !(a.skip && o != o);
    const double e = __builtin_sqrt(w) * d, ae = __builtin_fabs(e);
    const bool quad = ae <= a.delta;
    const double s = __builtin_sqrt(quad ? w : w * (a.delta / ae));
    slot_d = obs ? s * d : 0.0;
    slot_s = obs ? s : 0.0;
    lsum += obs ? (quad ? e * e : 2.0 * a.delta * ae - a.delta * a.delta) : 0.0;
}
// the rows of X scaled by the tile S (the s of a row broadcast over its columns): a select guards the product
PDP_DEV d4 wls_scale(const d4 S, const d4 X) {
    d4 Xm;
#pragma unroll
    for (int r = 0; r < 4; ++r) Xm[r] = S[r] != 0.0 ? S[r] * X[r] : 0.0;
    return Xm;
}


// ---- PDP_FUSED_GN_W: the run-time arguments of the OC units' weighted mode, one struct at the end of the kernels' argument list.  Neither pointer is ever NULL: without
// weights the host passes demo_x / demo_u (readable blocks of the same shape) and clears the bit of has_w, and the pass selects 1.0.
struct OcWls {
    const double* wx;           // [B or 1][T+1][NX]
    const double* wu;           // [B or 1][T][NU]
    long long bsx, bsu;         // (T+1) NX / T NU, or 0: one block shared by the batch
    double delta;               // Huber's threshold on the standardised residual; +inf: off
    int has_w, skip;            // bit 0: weights_x given, bit 1: weights_u given; PDP_GRAD_SKIP_MISSING
};
PDP_DEV SysidWls oc_wls_x(const OcWls a) { return SysidWls{a.wx, a.bsx, a.delta, a.has_w & 1, a.skip}; }
PDP_DEV SysidWls oc_wls_u(const OcWls a) { return SysidWls{a.wu, a.bsu, a.delta, (a.has_w >> 1) & 1, a.skip}; }
PDP_DEV OcWls oc_wls(const OcWls a) { return a; }              // the one element of the kernels' trailing pack

}  // namespace pdp
