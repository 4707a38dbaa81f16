// pdp_sysid_step_kernels.h - the fused SysID.step (reference PDP/PDP.py:1178-1296: integrateSys with the given controls, getAuxSys, integrateAuxSys
// X_{t+1} = F X_t + E, chain rule with the prediction error) and its two kernels in one place:
//     sysid_step_kernel    one wavefront per trajectory: the rollout (uniform, x kept in LDS), then the sweep over chunks of pool rows; GIVEN: the trajectory comes
//                          from sysid_integrate_kernel's pre-pass and stays in global memory;
//     sysid_step2_kernel   the two-wave pipeline of cp_step_poly2_kernel (pdp_cp_pair_kernels.h): wave R rolls out and publishes its progress, wave S follows a
//                          chunk behind with the same sweep.  Same arithmetic in the same order, bit for bit, in every mode (tests/test_gpu_cp_pair.py).
// Stated once for both: the slice (SysidLayout: the constants of the kernels' pointers and the host's word and row counts), the trailing argument pack (SysidArgs,
// sysid_arg, sysid_weights) and the rollout (sysid_rollout).  Every instantiation of both kernels compiles to the instructions it had with that text in place, to
// the same instructions in another order, or to those with a scalar compare and its branch complemented (profiles/sysid_shared_body_code_object_diff.txt).  What did NOT keep that as a helper stays in the kernels, side by side,
// each with a comment at its place: the pointers into the slice, the gather set, the lane-per-step row fill, the sensitivity step, the terminal row and the output
// row.  Besides them the kernels hold what differs between them: slot / bb arithmetic, which wave rolls, the synchronisation, GIVEN and the skeleton of the chunk loop.
// MODE: one of PDP_SYSID_* (pdp_chain_rule.h); everything here is forced inline and an instantiation contains only its own arms.
#pragma once
#include <tuple>
#include <type_traits>
#include "pdp_model_kernels.h"
#include "pdp_wave.h"

namespace pdp {

// ---- the trailing pack of the kernels and of the host's launch, fixed by MODE: x0 [B][NX] (every Gauss-Newton mode; NULL: x_obs[:, 0]), the mask of the estimated
// components of x0 (INI), the weights' arguments (WLS).  PDP_SYSID_PLAIN: empty - the plain kernels keep their argument list.
template <int MODE>
struct SysidArgsOf {
    using M = SysidMode<MODE, 1>;
    template <bool ON, class A> using opt = std::conditional_t<ON, std::tuple<A>, std::tuple<>>;
    using type = decltype(std::tuple_cat(opt<M::GN, const double*>{}, opt<M::INI, unsigned>{}, opt<M::WLS, SysidWls>{}));
};
template <int MODE> using SysidArgs = typename SysidArgsOf<MODE>::type;
// the host's tuple: each element of SysidArgs<MODE> taken by its type from what the entry point was given
template <int MODE>
__host__ inline SysidArgs<MODE> sysid_args(const double* x0, unsigned ini_mask, SysidWls wls) {
    const std::tuple<const double*, unsigned, SysidWls> all{x0, ini_mask, wls};
    return std::apply([&](auto... e) { return SysidArgs<MODE>{std::get<decltype(e)>(all)...}; }, SysidArgs<MODE>{});
}
// the element of type A of a kernel's pack: const double* is x0, unsigned the mask, SysidWls itself.  Absent: A{} (x0: nullptr)
template <class A>
PDP_DEV A sysid_arg() { return A{}; }
template <class A, class H, class... R>
PDP_DEV A sysid_arg(H h, R... r) {
    if constexpr (std::is_same_v<A, H>) return h;
    else return sysid_arg<A>(r...);
}

// ---- doubles of LDS per trajectory, in the slice's order:
// [cpool NC | pool `rows` rows of STRIDE | x (T+1) x NX | dlT DLT = NX + 1 (WLS: + NX) | u T x NU | dump DUMP = 64 + NX | hand-over counter, padding FL]
// given: the trajectory and the controls stay in global memory (no staging).  WLS: the scales s take a second group of NX slots of a pool row (DLS ..) beside the
// residuals (DLX ..), and the NX scales of the terminal row lie behind its residuals (dlT + DLT_S ..).  The kernels take every constant from here and add the parts
// to their pointers in their own text, the two run-time sizes (T + 1) NX and T NU spelled out: returned by a function of this struct, forced inline or not, they
// changed how the LDS addresses of every pair instantiation fold ((T + 1) NX split into T NX and an offset), and with it instructions outside the three classes.
template <class Mdl, int MODE>
struct SysidLayout {
    static constexpr bool WLS = SysidMode<MODE, 1>::WLS;
    static constexpr int NX = Mdl::NX, NU = Mdl::NU;
    static constexpr int NC = 1 + Mdl::PATH_NCONST, DLX = Mdl::PATH_NVAR, DLS = DLX + NX, STRIDE = (Mdl::PATH_NVAR + (WLS ? 2 : 1) * NX) | 1;
    static constexpr int DLT = NX + 1 + (WLS ? NX : 0), DLT_S = NX + 1, DUMP = 64 + NX, FL = 8;
    static constexpr int words(int T, int rows, bool given) {          // the host's count: the parts above, added up
        return (NC + rows * STRIDE + (given ? 0 : (T + 1) * NX) + DLT + (given ? 0 : T * NU) + DUMP + FL + 1) & ~1;
    }
};
template <class Mdl, int MODE>
__host__ inline int sysid_slice(int T, int rows = Mdl::CHUNK, bool given = false) { return SysidLayout<Mdl, MODE>::words(T, rows, given); }
// pool rows of the given-trajectory mode: what lets `wgs` workgroups (wavefronts) share a CU's 160 KB.  12 = three wavefronts per SIMD, what the 162 VGPRs of that
// instantiation allow (forced to 128 registers for four waves it spills 28); measured 8 / 12 / 16: 0.316 / 0.293 / 0.298 ms at B = 8192 (profiles/r04_rollout_prepass.txt)
template <class Mdl, int MODE>
__host__ inline int sysid_rows_given(int T, int wgs) {
    const int fit = (160 * 1024 / 8 / wgs - 64 - sysid_slice<Mdl, MODE>(T, 0, true)) / SysidLayout<Mdl, MODE>::STRIDE;
    return fit >= 4 ? (fit < Mdl::CHUNK ? fit : Mdl::CHUNK) : (Mdl::CHUNK < 4 ? Mdl::CHUNK : 4);
}
// Pool rows (stages per lane-parallel Jacobian pass) of sysid_step_kernel.  The generated CHUNK (a 17 KB pool for the quadrotor) makes a workgroup 31 KB: five
// wavefronts per CU - fine while there is at most one trajectory per SIMD.  A batch with several trajectories per SIMD (C5's total of 8192 on one GPU: eight rounds)
// is served better by TWO resident waves per SIMD that fill each other's latency gaps (two waves take 1.4x the time of one): the pool is
// cut to what lets eight workgroups share the CU's 160 KB.
template <class Mdl, int MODE>
__host__ inline int sysid_rows(int B, int T, int cus) {
    if (B <= 4 * cus) return Mdl::CHUNK;
    const int fit = (160 * 1024 / 8 / 8 - 64 - sysid_slice<Mdl, MODE>(T, 0, false)) / SysidLayout<Mdl, MODE>::STRIDE;      // (64 doubles of slack for the allocation granularity)
    return fit >= 4 ? (fit < Mdl::CHUNK ? fit : Mdl::CHUNK) : Mdl::CHUNK;
}

// WLS: the weights of trajectory b (every other mode: none)
template <class SM, class... Ini>
PDP_DEV const double* sysid_weights(int b, Ini... ini) {
    if constexpr (SM::WLS) return sysid_arg<SysidWls>(ini...).w + (int64_t)b * sysid_arg<SysidWls>(ini...).bstride;
    else return nullptr;
}

// ---- the rollout (uniform: the same value in every lane) of trajectory b into the staging xs.  It starts from x0 of the pack (GN; NULL or PLAIN:
// ini_state = batch_states[i][0] = ob[0 .. NX), PDP.py:1269).  u_t comes from the LDS staging `us`, requested one step ahead (read from global memory inside the loop
// every step waited for a round trip to memory); x_{t+1} goes to the staging from lane 0 without a conditional block - the other lanes store into `dump`
// (cp_step_poly_kernel).  PROGRESS: t + 1 into `fl` after every step, for the wave that follows, WITHOUT a branch or a wait: a plain LDS store behind the staging
// stores (see cp_step_poly2_kernel).  (Moved here the rollout kept its instructions, reordered; in the rocket's dynamics the compiler fuses another product of a sum
// a b + c d than it did in the kernels' text - the same in both kernels.)
template <class Mdl, bool GN, bool PROGRESS, class... Ini>
PDP_DEV void sysid_rollout(int T, int lane, int b, const double* ob, const double* th, const double* pc, double* xs, const double* us, double* dump,
                           [[maybe_unused]] int* fl, Ini... ini) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU;
    double xc[NX], xn[NX], uc[NU], un[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) xc[i] = ob[i];
    if constexpr (GN) {
        if (const double* x0 = sysid_arg<const double*>(ini...)) {
#pragma unroll
            for (int i = 0; i < NX; ++i) xc[i] = x0[(int64_t)b * NX + i];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) xs[i] = xc[i];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) un[i] = us[i];
    for (int t = 0; t < T; ++t) {
        const int tn = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int i = 0; i < NU; ++i) { uc[i] = un[i]; un[i] = us[tn * NU + i]; }
        Mdl::dyn(xc, uc, th, pc, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) xc[i] = xn[i];
        double* dx_ = lane == 0 ? xs + (t + 1) * NX : dump + lane;
#pragma unroll
        for (int i = 0; i < NX; ++i) dx_[i] = xn[i];
        if constexpr (PROGRESS) {
            asm volatile("" ::: "memory");
            __hip_atomic_store(fl, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// Fused SysID.step, one wavefront per trajectory.  pdp_sysid_step_gn_batched selects PDP_SYSID_GN / PDP_SYSID_GN_MISS, pdp_sysid_step_gn_ini_batched
// PDP_SYSID_GN_INI / PDP_SYSID_GN_INI_MISS, pdp_sysid_step_wls_batched PDP_SYSID_GN_W / PDP_SYSID_GN_W_INI.
// xgiven [B][T+1][NX] (GIVEN): the trajectory, rolled out beforehand by sysid_integrate_kernel with ONE LANE per trajectory - the mode for batches with several
// trajectories per SIMD: the rollout here runs one trajectory on all 64 lanes (the same value in every lane), which is the right thing while the SIMD has nothing
// else to do and 63/64 wasted once other trajectories wait for it (C5a's 8192 on one GPU: 8 rounds of a 26 us rollout against one 21 us pass for all of them)
template <class Mdl, int NT, bool GIVEN = false, int MODE = PDP_SYSID_PLAIN, class... Ini>
__global__ void __launch_bounds__(64) sysid_step_kernel(int B, int T, const double* __restrict__ u, const double* __restrict__ xobs,
                                                         const double* __restrict__ theta, int tb, double* __restrict__ loss, double* __restrict__ grad, int CH,
                                                         const double* __restrict__ xgiven_, Ini... ini) {
    using SM = SysidMode<MODE, NT>;
    using L = SysidLayout<Mdl, MODE>;
    static_assert(std::is_same_v<std::tuple<Ini...>, SysidArgs<MODE>>, "the trailing pack is SysidArgs<MODE>");
    const double* __restrict__ xgiven = GIVEN ? xgiven_ : nullptr;      // (a template parameter: each instantiation keeps its own register allocation)
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* blk = lds;                       // SysidLayout's parts, added up in this kernel's own text (see there)
    double* pool = blk + L::NC;
    double* xs = pool + CH * L::STRIDE;      // (T+1) x NX   (not in the given-trajectory mode: stages are evaluated from global memory there)
    double* dlT = xs + (xgiven ? 0 : (T + 1) * NX);
    double* us = dlT + L::DLT;               // T x NU: the given controls, staged once with coalesced loads (rollout mode only)
    double* dump = us + (xgiven ? 0 : T * NU);      // words nobody reads (see the rollout)
    const int b = blockIdx.x, lane = threadIdx.x;
    double th[NP];
    load_theta<Mdl>(theta, b, tb, th);
    double pc[Mdl::NPC];
    Mdl::precompute(th, pc);
    const double* ub = u + (int64_t)b * T * NU;
    const double* ob = xobs + (int64_t)b * (T + 1) * NX;
    const double* wb = sysid_weights<SM>(b, ini...);
    if (lane == 0) blk[0] = 0.0;
    for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
    const double* xg = xgiven ? xgiven + (int64_t)b * (T + 1) * NX : nullptr;
    if (!xgiven) for (int q = lane; q < T * NU; q += 64) us[q] = ub[q];
    __syncthreads();
    if constexpr (!GIVEN) sysid_rollout<Mdl, SM::GN, false>(T, lane, b, ob, th, pc, xs, us, dump, nullptr, ini...);
    __syncthreads();
    // the gather set, in this kernel's own text: built in a helper it changed vector instructions of every instantiation that called it
    Gather gFT, gDX, gE[NT];
    make_gather(gFT, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX && c < NX) ? Mdl::path_code(0, c * NX + r) : -1; });
    make_gather(gDX, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX) ? L::DLX + r : -1; });
    [[maybe_unused]] Gather gS;                            // WLS: the scales s of the rows
    if constexpr (SM::WLS) make_gather(gS, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX) ? L::DLS + r : -1; });
#pragma unroll
    for (int j = 0; j < NT; ++j)
        make_gather(gE[j], lane, L::NC, L::STRIDE, [j](int r, int c) { return (r < NX && 16 * j + c < NP) ? Mdl::path_code(1, r * NP + 16 * j + c) : -1; });
    const d4 z = zero4();
    d4 X[NT];
    double acc[NT], lsum = 0.0;
    [[maybe_unused]] d4 Gn = z;                            // GN: sum_t X_t' X_t
#pragma unroll
    for (int j = 0; j < NT; ++j) { X[j] = z; acc[j] = 0.0; }
    if constexpr (SM::INI) X[0] = sysid_ini_tile<NX, NP>(lane, sysid_arg<unsigned>(ini...));      // X_0: the unit columns of the estimated components of x0
    const int nchunk = (T + CH - 1) / CH;
    const int ch = (T + nchunk - 1) / nchunk;      // chunks of equal length
    for (int c = 0; c < nchunk; ++c) {
        const int t0 = c * ch, cnt = min(ch, T - t0);
        __syncthreads();
        if (lane < cnt) {                   // the row fill, in this kernel's own text: with x_t and u_t handed to a helper through a callable (xg or xs, ub or us) the GIVEN
            const int t = t0 + lane;        // instantiations lost their branches on xg and 60 to 220 instructions; so did the terminal row below
            double xc[NX], uc[NU];
            double* row = pool + lane * L::STRIDE;
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                xc[i] = xg ? xg[t * NX + i] : xs[t * NX + i];
                if constexpr (SM::WLS) wls_slot(row[L::DLX + i], row[L::DLS + i], xc[i], ob[t * NX + i], wb[t * NX + i], sysid_arg<SysidWls>(ini...), lsum);
                else residual_slot<SM::RES>(row[L::DLX + i], xc[i], ob[t * NX + i], lsum);
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) uc[i] = xg ? ub[t * NU + i] : us[t * NU + i];
            PackedSink s{row};
            Mdl::eval_path(xc, uc, nullptr, th, pc, s);
        }
        __syncthreads();
        for (int tl = 0; tl < cnt; ++tl) {            // the sensitivity step, in this kernel's own text: as a helper it changed which product of contract_step the compiler
            d4 FT = gather_tile(blk, gFT, tl);        // rounds on its own (the other three are fused) in 27 of 84 instantiations - the last bits of the gradient
            d4 DX = gather_tile(blk, gDX, tl);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                d4 E = gather_tile(blk, gE[j], tl);
                if constexpr (SM::WLS) {          // DX carries s d, Xm = s X: grad += (s d)' (s X), G += (s X)' (s X)
                    const d4 Xm = wls_scale(gather_tile(blk, gS, tl), X[j]);
                    acc[j] += contract_step(DX, Xm);
                    Gn = gram_add<false>(Xm, Gn);
                } else
                if constexpr (SM::MISS) {         // (pdp_chain_rule.h: mask_step, in this kernel's own text; NT == 1)
                    d4 Xm;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const bool obs = DX[r] == DX[r]; Xm[r] = obs ? X[j][r] : 0.0; DX[r] = obs ? DX[r] : 0.0; }
                    acc[j] += contract_step(DX, Xm);
                    Gn = gram_add<false>(Xm, Gn);
                } else {
                acc[j] += contract_step(DX, X[j]);
                if constexpr (SM::GN) Gn = gram_add<false>(X[j], Gn);
                }
                X[j] = mma_tn(FT, X[j], E);
            }
        }
    }
    __syncthreads();
    if (lane < NX) {
        if constexpr (SM::WLS) wls_slot(dlT[lane], dlT[L::DLT_S + lane], xg ? xg[T * NX + lane] : xs[T * NX + lane], ob[T * NX + lane], wb[T * NX + lane], sysid_arg<SysidWls>(ini...), lsum);
        else
        if constexpr (SM::MISS) { const double o = ob[T * NX + lane]; residual_slot<SM::RES>(dlT[lane], xg ? xg[T * NX + lane] : xs[T * NX + lane], o, lsum); }      // (x_obs first, as it always was here)
        else residual_slot<SM::RES>(dlT[lane], xg ? xg[T * NX + lane] : xs[T * NX + lane], ob[T * NX + lane], lsum);
    }
    __syncthreads();
    // the output row, in this kernel's own text: as a helper with the store predicate as its argument it changed vector compares, selects and waits of the
    // Gauss-Newton instantiations (the addresses of the packed row were formed in it)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = tile_row(lane, r);
            if constexpr (SM::WLS) { if (row < NX) { const double sT = dlT[L::DLT_S + row]; X[j][r] = sT != 0.0 ? sT * X[j][r] : 0.0; acc[j] += dlT[row] * X[j][r]; } }      // (X_T scaled in place)
            else
            if (row < NX) { const double d = dlT[row]; X[j][r] = observed<SM::MISS>(d, X[j][r]); acc[j] += observed<SM::MISS>(d, d) * X[j][r]; }      // (MISS: X_T masked in place)
        }
        double a = sum_over_rowgroups(acc[j]);
        if constexpr (SM::INI) {                           // the row of W = p + q unknowns: grad [W] | loss | G [W][W]
            const int W = sysid_ini_width<NP>(sysid_arg<unsigned>(ini...));
            double* row = grad + (int64_t)b * (W + 1 + W * W);
            if (lane < W) row[lane] = a;
            Gn = gram_add<false>(X[j], Gn);                // X_T
            sysid_ini_store(row + W + 1, W, lane, Gn);
        } else if constexpr (SM::GN) {
            if (lane < NP) grad[(int64_t)b * (NP + 1 + NP * NP) + lane] = a;
            Gn = gram_add<false>(X[j], Gn);                // X_T
            store_dense(grad + (int64_t)b * (NP + 1 + NP * NP) + NP + 1, NP, NP, NP, 0, 0, lane, Gn);
        } else {
        if (lane < 16 && 16 * j + lane < NP) grad[(int64_t)b * NP + 16 * j + lane] = a;
        }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) loss[b] = lsum;
    if constexpr (SM::INI) { const int W = sysid_ini_width<NP>(sysid_arg<unsigned>(ini...)); if (lane == 0) grad[(int64_t)b * (W + 1 + W * W) + W] = lsum; }
    else
    if constexpr (SM::GN) { if (lane == 0) grad[(int64_t)b * (NP + 1 + NP * NP) + NP] = lsum; }
}

// ... and as the two-wave pipeline: wave R rolls the model out along the recorded controls, wave S follows a chunk behind with the Jacobians, the prediction
// errors and the sensitivity recursion.  TPW trajectories per workgroup; `slice`: SysidLayout's words of one of them.
template <class Mdl, int NT, int TPW, int MODE = PDP_SYSID_PLAIN, class... Ini>
__global__ void __launch_bounds__(128 * TPW) sysid_step2_kernel(int B, int T, const double* __restrict__ u, const double* __restrict__ xobs,
                                                                 const double* __restrict__ theta, int tb, double* __restrict__ loss, double* __restrict__ grad, int slice,
                                                                 Ini... ini) {
    using SM = SysidMode<MODE, NT>;
    using L = SysidLayout<Mdl, MODE>;
    static_assert(std::is_same_v<std::tuple<Ini...>, SysidArgs<MODE>>, "the trailing pack is SysidArgs<MODE>");
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NP, CH = Mdl::CHUNK;
    static_assert(TPW == 1 || TPW == 2 || TPW == 4, "trajectories per workgroup");
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, slot = wid & (TPW - 1);
    const bool roller = wid < TPW;
    const int b = blockIdx.x * TPW + slot;
    const int bb = b < B ? b : B - 1;                         // (a workgroup's spare slots repeat the last trajectory and store nothing)
    const bool mine = b < B;
    double* blk = lds_all + (size_t)slot * slice;             // SysidLayout's parts, added up in this kernel's own text (see there)
    double* pool = blk + L::NC;
    double* xs = pool + CH * L::STRIDE;
    double* dlT = xs + (T + 1) * NX;
    double* us = dlT + L::DLT;
    double* dump = us + T * NU;
    int* fl = (int*)(dump + L::DUMP);        // stages rolled out so far
    const double* ub = u + (int64_t)bb * T * NU;
    const double* ob = xobs + (int64_t)bb * (T + 1) * NX;
    const double* wb = sysid_weights<SM>(bb, ini...);
    if (roller) {
        if (lane == 0) { blk[0] = 0.0; fl[0] = 0; }
        for (int i_ = lane; i_ < Mdl::PATH_NCONST; i_ += 64) blk[1 + i_] = Mdl::path_const(i_);
        for (int q = lane; q < T * NU; q += 64) us[q] = ub[q];
    }
    __syncthreads();                                          // the only workgroup barrier: constants, controls and the zeroed counter
    double th[NP];
    load_theta<Mdl>(theta, bb, tb, th);
    double pc[Mdl::NPC];
    Mdl::precompute(th, pc);
    if (roller) {
        sysid_rollout<Mdl, SM::GN, true>(T, lane, bb, ob, th, pc, xs, us, dump, fl, ini...);
    } else {
        // the gather set, in this kernel's own text (as in sysid_step_kernel)
        Gather gFT, gDX, gE[NT];
        make_gather(gFT, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX && c < NX) ? Mdl::path_code(0, c * NX + r) : -1; });
        make_gather(gDX, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX) ? L::DLX + r : -1; });
        [[maybe_unused]] Gather gS;                        // WLS: the scales s of the rows
        if constexpr (SM::WLS) make_gather(gS, lane, L::NC, L::STRIDE, [](int r, int c) { return (r < NX) ? L::DLS + r : -1; });
#pragma unroll
        for (int j = 0; j < NT; ++j)
            make_gather(gE[j], lane, L::NC, L::STRIDE, [j](int r, int c) { return (r < NX && 16 * j + c < NP) ? Mdl::path_code(1, r * NP + 16 * j + c) : -1; });
        const d4 z = zero4();
        d4 X[NT];
        double acc[NT], lsum = 0.0;
        [[maybe_unused]] d4 Gn = z;                            // GN: sum_t X_t' X_t
#pragma unroll
        for (int j = 0; j < NT; ++j) { X[j] = z; acc[j] = 0.0; }
        if constexpr (SM::INI) X[0] = sysid_ini_tile<NX, NP>(lane, sysid_arg<unsigned>(ini...));      // X_0: the unit columns of the estimated components of x0
        const int nchunk = (T + CH - 1) / CH;
        const int ch = (T + nchunk - 1) / nchunk;
        for (int c = 0; c < nchunk; ++c) {
            const int t0 = c * ch, cnt = min(ch, T - t0);
            wg_wait_ge(fl, t0 + cnt);                        // x_t of the chunk's stages are in the staging (x_{t0+cnt-1} was stored by step t0+cnt-2; the counter is past it)
            wave_lds_sync();
            if (lane < cnt) {               // the row fill, in this kernel's own text (as in sysid_step_kernel; here the helper added waits)
                const int t = t0 + lane;
                double xc[NX], uc[NU];
                double* row = pool + lane * L::STRIDE;
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    xc[i] = xs[t * NX + i];
                    if constexpr (SM::WLS) wls_slot(row[L::DLX + i], row[L::DLS + i], xc[i], ob[t * NX + i], wb[t * NX + i], sysid_arg<SysidWls>(ini...), lsum);
                    else residual_slot<SM::RES>(row[L::DLX + i], xc[i], ob[t * NX + i], lsum);
                }
#pragma unroll
                for (int i = 0; i < NU; ++i) uc[i] = us[t * NU + i];
                PackedSink s{row};
                Mdl::eval_path(xc, uc, nullptr, th, pc, s);
            }
            wave_lds_sync();
            for (int tl = 0; tl < cnt; ++tl) {            // the sensitivity step, in this kernel's own text (as in sysid_step_kernel)
                d4 FT = gather_tile(blk, gFT, tl);
                d4 DX = gather_tile(blk, gDX, tl);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    d4 E = gather_tile(blk, gE[j], tl);
                    if constexpr (SM::WLS) {          // DX carries s d, Xm = s X: grad += (s d)' (s X), G += (s X)' (s X)
                        const d4 Xm = wls_scale(gather_tile(blk, gS, tl), X[j]);
                        acc[j] += contract_step(DX, Xm);
                        Gn = gram_add<false>(Xm, Gn);
                    } else
                    if constexpr (SM::MISS) {         // (pdp_chain_rule.h: mask_step, in this kernel's own text; NT == 1)
                        d4 Xm;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const bool obs = DX[r] == DX[r]; Xm[r] = obs ? X[j][r] : 0.0; DX[r] = obs ? DX[r] : 0.0; }
                        acc[j] += contract_step(DX, Xm);
                        Gn = gram_add<false>(Xm, Gn);
                    } else {
                    acc[j] += contract_step(DX, X[j]);
                    if constexpr (SM::GN) Gn = gram_add<false>(X[j], Gn);
                    }
                    X[j] = mma_tn(FT, X[j], E);
                }
            }
        }
        wg_wait_ge(fl, T);                                   // x_T
        wave_lds_sync();
        if (lane < NX) {
            if constexpr (SM::WLS) wls_slot(dlT[lane], dlT[L::DLT_S + lane], xs[T * NX + lane], ob[T * NX + lane], wb[T * NX + lane], sysid_arg<SysidWls>(ini...), lsum);
            else
            if constexpr (SM::MISS) { const double o = ob[T * NX + lane]; residual_slot<SM::RES>(dlT[lane], xs[T * NX + lane], o, lsum); }      // (x_obs first, as in sysid_step_kernel)
            else residual_slot<SM::RES>(dlT[lane], xs[T * NX + lane], ob[T * NX + lane], lsum);
        }
        wave_lds_sync();
        // the output row, in this kernel's own text (as in sysid_step_kernel), every store under `mine`
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(lane, r);
                if constexpr (SM::WLS) { if (row < NX) { const double sT = dlT[L::DLT_S + row]; X[j][r] = sT != 0.0 ? sT * X[j][r] : 0.0; acc[j] += dlT[row] * X[j][r]; } }      // (X_T scaled in place)
                else
                if constexpr (SM::MISS) {              // (observed(), in this kernel's own text: through sysid_step_kernel's spelling the skip-missing instantiations of this kernel gained a select, and four changed their fp64 instructions)
                    if (row < NX) { const double d = dlT[row]; const bool obs = d == d; X[j][r] = obs ? X[j][r] : 0.0; acc[j] += (obs ? d : 0.0) * X[j][r]; }
                } else {
                if (row < NX) acc[j] += dlT[row] * X[j][r];
                }
            }
            double a = sum_over_rowgroups(acc[j]);
            if constexpr (SM::INI) {                       // the row of W = p + q unknowns: grad [W] | loss | G [W][W]
                Gn = gram_add<false>(X[j], Gn);            // X_T
                if (mine) {
                    const int W = sysid_ini_width<NP>(sysid_arg<unsigned>(ini...));
                    double* row = grad + (int64_t)b * (W + 1 + W * W);
                    if (lane < W) row[lane] = a;
                    sysid_ini_store(row + W + 1, W, lane, Gn);
                }
            } else if constexpr (SM::GN) {
                Gn = gram_add<false>(X[j], Gn);            // X_T
                if (mine) {
                    if (lane < NP) grad[(int64_t)b * (NP + 1 + NP * NP) + lane] = a;
                    store_dense(grad + (int64_t)b * (NP + 1 + NP * NP) + NP + 1, NP, NP, NP, 0, 0, lane, Gn);
                }
            } else {
            if (mine && lane < 16 && 16 * j + lane < NP) grad[(int64_t)b * NP + 16 * j + lane] = a;
            }
        }
        lsum = wave_sum(lsum);
        if (mine && lane == 0) loss[b] = lsum;
        if constexpr (SM::INI) { const int W = sysid_ini_width<NP>(sysid_arg<unsigned>(ini...)); if (mine && lane == 0) grad[(int64_t)b * (W + 1 + W * W) + W] = lsum; }
        else
        if constexpr (SM::GN) { if (mine && lane == 0) grad[(int64_t)b * (NP + 1 + NP * NP) + NP] = lsum; }
    }
}

}  // namespace pdp
