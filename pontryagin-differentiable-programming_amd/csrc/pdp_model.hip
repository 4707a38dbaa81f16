// pdp_model.hip - C-ABI entry points of one generated model library (libpdp_model_<name>.so), section B of
// include/pdp_hip.h.  Compiled once per model with -DPDP_MODEL_HEADER="generated/<name>.h" (codegen.py).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <tuple>
#include "../../include/pdp_hip.h"
#include "../../include/pdp_hip_sysid_gn.h"
#include "../../include/pdp_hip_sysid_ini.h"
#include "../../include/pdp_hip_sysid_wls.h"
#include "../../include/pdp_hip_oc_wls.h"
#include "../../include/pdp_hip_sysid_vjp.h"
#include "../../include/pdp_hip_sysid_vjp_u.h"
#include "../../include/pdp_hip_sysid_jvp.h"
#ifndef PDP_MODEL_HEADER
#error "compile with -DPDP_MODEL_HEADER=\"generated/<model>.h\""
#endif
#define PDP_HD __host__ __device__ inline
#include PDP_MODEL_HEADER
#ifdef PDP_PHASE_TIMING_FINE      // timing builds with -DPDP_PHASE_TIMING_FINE: cycle stamps inside the Riccati step of the fused3 runner (probes/phase_timing3.py)
namespace pdp { extern __device__ long long g_rb_stamp[16]; }
#define PDP_RB_T(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) pdp::g_rb_stamp[i] = __builtin_readcyclecounter(); } while (0)
#endif
#include "pdp_model_kernels.h"
#include "pdp_lqr_kernels.h"
#include "pdp_ocsolve_kernels.h"
#include "pdp_ocsolve2_kernels.h"
#include "pdp_cp_mlp_kernels.h"
#include "pdp_fused3_kernels.h"
#include "pdp_cp_pair_kernels.h"
#include "pdp_sysid_step_kernels.h"
#include "pdp_cp_generic_kernels.h"
#include "pdp_sysid_vjp_kernels.h"
#include "pdp_sysid_jvp_kernels.h"
#include "pdp_oc_x0_vjp_kernels.h"
#include "pdp_cp_vjp_kernels.h"
#include "pdp_cp_jvp_kernels.h"
#include "pdp_launch.h"

using namespace pdp;

#ifndef PDP_FUSED_DEFAULT_VARIANT
#define PDP_FUSED_DEFAULT_VARIANT 3
#endif

namespace {

inline hipStream_t S(void* s) { return (hipStream_t)s; }

[[maybe_unused]] inline int device_cu_count() {
    static int n = 0;
    if (n == 0) { int dev = 0; (void)hipGetDevice(&dev); if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256; }
    return n;
}

template <class Mdl> constexpr bool fused_oc_ok() { return Mdl::KIND == PDP_KIND_OC && Mdl::NX <= 16 && Mdl::NU <= 4 && Mdl::NU + Mdl::NP <= 16; }

template <class Mdl>
int64_t oc_ws_bytes(int B, int T) {
    return (int64_t)B * T * fused_gain_doubles<Mdl>() * (int64_t)sizeof(double);
}

template <class Mdl>
int oc_rollout(int B, int T, const double* x0, const double* u, const double* th, int tb, double* x, double* cost, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        if (B <= 0 || T <= 0 || !x0 || !u || !th || !x) return PDP_E_ARG;
        return launch(oc_rollout_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, x0, u, th, tb, x, cost);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int oc_rollout_fb(int B, int T, const double* x0, const double* ubar, const double* xbar, const double* gains, const double* alpha, const double* th,
                  int tb, double* x, double* u, double* cost, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        if (B <= 0 || T <= 0 || !x0 || !ubar || !xbar || !gains || !alpha || !th || !x || !u || !cost) return PDP_E_ARG;
        return launch(oc_rollout_feedback_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, x0, ubar, xbar, gains, alpha, th, tb, x, u, cost);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int oc_ms_residuals(int B, int T, const double* x, const double* u, const double* lam, const double* th, int tb, double* c, double* rx, double* ru, double* cost,
                    void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        if (B <= 0 || T <= 0 || !x || !u || !lam || !th || !c || !rx || !ru || !cost) return PDP_E_ARG;
        const int64_t nthr = (int64_t)B * (T + 1);
        return launch(oc_ms_residuals_kernel<Mdl>, dim3((unsigned)((nthr + 63) / 64)), dim3(64), 0, S(st), B, T, x, u, lam, th, tb, c, rx, ru, cost);
    } else return PDP_E_MODE;
}
template <class Mdl>
int oc_costate(int B, int T, const double* x, const double* u, const double* th, int tb, double* lam, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        if (B <= 0 || T <= 0 || !x || !u || !th || !lam) return PDP_E_ARG;
        return launch(oc_costate_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, x, u, th, tb, lam);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int oc_auxsys(int B, int T, const double* x, const double* u, const double* lam, const double* th, int tb, const pdp_oc_auxsys* o, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        if (B <= 0 || T <= 0 || !x || !u || !lam || !th || !o) return PDP_E_ARG;
        const int nchunk = (T + auxsys_chunk<Mdl>() - 1) / auxsys_chunk<Mdl>();
        return launch(oc_auxsys_kernel<Mdl>, dim3((unsigned)((int64_t)B * (nchunk + 1))), dim3(64), 0, S(st), B, T, x, u, lam, th, tb, *o);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int oc_predict(int B, int T, const double* dth, int dtb, const double* dxdp, const double* dudp, const double* ric, double* x, double* u, double* lam, void* st) {
    if constexpr (fused_oc_ok<Mdl>()) {
        if (B <= 0 || T <= 0 || !dth || !dxdp || !dudp || !x || !u || (ric && !lam)) return PDP_E_ARG;
        return launch(oc_predict_kernel<Mdl>, dim3((unsigned)((int64_t)B * ((T + 3) / 4))), dim3(64), 0, S(st), B, T, dth, dtb, dxdp, dudp, ric, x, u, lam);
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}

template <class Mdl>
int oc_predict_rec(int B, int T, const double* dth, int dtb, const float* rec, double* x, double* u, double* lam, void* st) {
    if constexpr (fused_oc_ok<Mdl>()) {
        if (B <= 0 || T <= 0 || !dth || !rec || !x || !u) return PDP_E_ARG;
        return launch(oc_predict_rec_kernel<Mdl>, dim3((unsigned)((int64_t)B * ((T + 3) / 4))), dim3(64), 0, S(st), B, T, dth, dtb, rec, x, u, lam);
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}
// the instantiations of the two fused OC kernels, PDP_FUSED_PLAIN last: with_int's fallback
template <class F>
inline int with_fused_mode(int mode, F&& f) { return with_int<PDP_FUSED_RIC, PDP_FUSED_COT, PDP_FUSED_GN, PDP_FUSED_MISS, PDP_FUSED_GN_MISS, PDP_FUSED_PLAIN>(mode, f); }

// The launch of the fused OC unit, shared by its entry points (oc_pdp, oc_pdp_wls): PDP_E_SIZE where the horizon's staging exceeds the LDS, else the kernel variant
// with its geometry.  XW: the extra words of the forward row in the caller's layout.  run(kernel, workgroups, threads, LDS bytes) launches with the caller's
// arguments; pair(K, go) and wave(go) call go(kernel) with the caller's instantiation of oc_pdp_fused3_kernel for K trajectories per workgroup / of
// oc_pdp_fused_kernel.
// Kernel variants (environment PDP_FUSED_VARIANT overrides the default): 3 = runner / evaluator wave pair per trajectory, four
// trajectories per 512-thread workgroup (pdp_fused3_kernels.h) - the default wherever it applies (n > 4, rollout staging within the
// pool area); 1 = one wavefront per trajectory (systems with n <= 4, long horizons)
template <class Mdl, int XW, class Run, class Pair, class Wave>
int oc_pdp_launch(int B, int T, Run&& run, Pair&& pair, Wave&& wave) {
    const size_t lds = fused_lds_bytes<Mdl, XW>(T);
    if (lds > 160 * 1024) return PDP_E_SIZE;
    static const int variant = env_int("PDP_FUSED_VARIANT", PDP_FUSED_DEFAULT_VARIANT);
    if constexpr (Mdl::NX > 4) {
        if (variant == 3 && fused3_ok<Mdl, XW>(T)) {
            static const int tpw_env = env_int("PDP_FUSED_TPW", 0);          // (overrides the batch rule)
            const int tpw = tpw_env ? tpw_env : traj_per_workgroup(B, device_cu_count(), 4);
            return with_int<1, 2, 4>(tpw, [&](auto K) { return pair(K, [&](auto kern) { return run(kern, (B + K() - 1) / K(), 128 * K(), K() * 40 * 1024); }); });
        }
    }
    return wave([&](auto kern) { return run(kern, B, 64, lds); });
}

template <class Mdl>
int oc_pdp(int B, int T, int flags, const double* x0, const double* u, const double* th, int tb, const double* dx, const double* du, double* x,
           double* lam, double* loss, double* grad, double* dxdp, double* dudp, double* ric, float* prec, int32_t* status, void* ws, int64_t wsb, void* st) {
    if constexpr (fused_oc_ok<Mdl>()) {
        const bool cot = (flags & PDP_OC_COTANGENT) != 0;   // dx, du carry the cotangents of a caller's loss: no loss output, plain gradient only
        const bool gn = (flags & PDP_GRAD_GAUSS_NEWTON) != 0;   // grad is the packed row gradient | loss | G = J'J: plain gradient of the demonstration loss only
        const bool miss = (flags & PDP_GRAD_SKIP_MISSING) != 0;   // a NaN in dx / du is an entry that was not observed: plain or Gauss-Newton unit, no sensitivity output
        const bool records = ric || prec, sens = records || dxdp || dudp;          // the Riccati / prediction records; any sensitivity output
        if (B <= 0 || T <= 0 || !u || !th || !dx || !du || !x || !lam || (!loss && !cot) || !grad || !ws) return PDP_E_ARG;
        if ((cot || gn) && (sens || (flags & PDP_OC_PACKED) || (cot && gn))) return PDP_E_ARG;
        if (miss && (cot || sens)) return PDP_E_ARG;
        if (!(flags & PDP_OC_GIVEN_TRAJ) && !x0) return PDP_E_ARG;
        if (wsb < oc_ws_bytes<Mdl>(B, T)) return PDP_E_ARG;
        // the instantiation (a kernel's MODE): with records - and, fused3 only, with any sensitivity output - the one that writes them with buffer stores
        auto mode = [&](bool rec) {
            return rec ? PDP_FUSED_RIC : (cot ? PDP_FUSED_COT : (gn ? (miss ? PDP_FUSED_GN_MISS : PDP_FUSED_GN) : (miss ? PDP_FUSED_MISS : PDP_FUSED_PLAIN)));
        };
        auto run = [&](auto kern, int wgs, int threads, size_t lds_bytes) {
            return launch(kern, dim3(wgs), dim3(threads), lds_bytes, S(st), B, T, flags, x0, u, th, tb, dx, du, x, lam, loss, grad, dxdp, dudp, status, (double*)ws, ric, prec);
        };
        return oc_pdp_launch<Mdl, 0>(B, T, run,
                                     [&](auto K, auto&& go) { return with_fused_mode(mode(sens), [&](auto MODE) { return go(oc_pdp_fused3_kernel<Mdl, K(), MODE()>); }); },
                                     [&](auto&& go) { return with_fused_mode(mode(records), [&](auto MODE) { return go(oc_pdp_fused_kernel<Mdl, MODE()>); }); });
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}

// pdp_oc_sens_out.grad_x0: the fused unit's launch as it is, and behind it on the same stream the adjoint sweep of pdp_oc_x0_vjp_kernels.h on what that launch left in
// x and in the gain workspace.  Refused with the Gauss-Newton row and with missing observations before anything is launched; every other check, and PDP_E_SIZE, are
// the fused launch's own (the sweep's pool is at most SWEEP_POOL_DOUBLES: it never adds a size limit).
template <class Mdl>
int oc_pdp_x0(int B, int T, int flags, const double* x0, const double* u, const double* th, int tb, const double* dx, const double* du, double* x, double* lam,
              double* loss, double* grad, const pdp_oc_sens_out& so, int32_t* status, void* ws, int64_t wsb, void* st) {
    if (flags & (PDP_GRAD_GAUSS_NEWTON | PDP_GRAD_SKIP_MISSING)) return PDP_E_ARG;
    const int rc = oc_pdp<Mdl>(B, T, flags, x0, u, th, tb, dx, du, x, lam, loss, grad, so.dxdp, so.dudp, so.riccati, so.predict_record, status, ws, wsb, st);
    if (rc != 0) return rc;
    if constexpr (fused_oc_ok<Mdl>()) {
        if (wsb < oc_ws_bytes<Mdl>(B, T)) return PDP_E_ARG;        // (the gains the sweep reads)
        constexpr int rows = oc_x0_vjp_rows_of(OcX0VjpPool<Mdl>::STRIDE);
        return with_bool((flags & PDP_OC_COTANGENT) != 0, [&](auto COT) {
            return launch(oc_x0_vjp_kernel<Mdl, COT()>, dim3(B), dim3(64), sizeof(double) * (size_t)OcX0VjpPool<Mdl>::slice(rows), S(st), B, T, (const double*)x, u, th, tb,
                          dx, du, (const double*)ws, so.grad_x0, rows);
        });
    } else { return rc; }
}

// pdp_oc_pdp_grad_wls_batched (include/pdp_hip_oc_wls.h): the PDP_FUSED_GN_W instantiations, chosen by oc_pdp_launch with the mode's own (longer) layout.  The checks
// come in the order of the header.
template <class Mdl>
int oc_pdp_wls(int B, int T, int flags, const double* x0, const double* u, const double* th, int tb, const double* dx, const double* du, const double* wx, int64_t wxs,
               const double* wu, int64_t wus, double delta, double* x, double* lam, double* loss, double* packed, int32_t* status, void* ws, int64_t wsb, void* st) {
    if constexpr (fused_oc_ok<Mdl>()) {
        constexpr int XW = Mdl::NX + Mdl::NU;                // the forward row's extra words
        if (flags & ~(PDP_OC_GIVEN_TRAJ | PDP_GRAD_SKIP_MISSING)) return PDP_E_ARG;
        if (!(delta > 0.0)) return PDP_E_ARG;                // (<= 0 and NaN)
        if (wxs != 0 && wxs != (int64_t)(T + 1) * Mdl::NX) return PDP_E_ARG;
        if (wus != 0 && wus != (int64_t)T * Mdl::NU) return PDP_E_ARG;
        if (!u || !th || !dx || !du || !x || !lam || !loss || !packed || !status || !ws) return PDP_E_ARG;
        if (!(flags & PDP_OC_GIVEN_TRAJ) && !x0) return PDP_E_ARG;
        if (B <= 0 || T <= 0) return PDP_E_ARG;
        if (wsb < oc_ws_bytes<Mdl>(B, T)) return PDP_E_ARG;
        // without weights the kernels load the demonstrations in their place (readable blocks of the same shape) and select 1.0
        const OcWls a{wx ? wx : dx, wu ? wu : du, wx ? (long long)wxs : (long long)(T + 1) * Mdl::NX, wu ? (long long)wus : (long long)T * Mdl::NU, delta,
                      (wx ? 1 : 0) | (wu ? 2 : 0), (flags & PDP_GRAD_SKIP_MISSING) ? 1 : 0};
        double* const no_sens = nullptr;
        float* const no_rec = nullptr;
        auto run = [&](auto kern, int wgs, int threads, size_t lds_bytes) {
            return launch(kern, dim3(wgs), dim3(threads), lds_bytes, S(st), B, T, flags, x0, u, th, tb, dx, du, x, lam, loss, packed, no_sens, no_sens, status, (double*)ws,
                          no_sens, no_rec, a);
        };
        return oc_pdp_launch<Mdl, XW>(B, T, run, [&](auto K, auto&& go) { return go(oc_pdp_fused3_kernel<Mdl, K(), PDP_FUSED_GN_W, OcWls>); },
                                      [&](auto&& go) { return go(oc_pdp_fused_kernel<Mdl, PDP_FUSED_GN_W, OcWls>); });
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}

// ---- batched Newton solve (pdp_oc_solve_batched): workspace carve-up and the iteration loop ---------------------------------
template <class Mdl>
struct OcSolveWs {
    double *lam_eff, *F, *G, *Hxx, *Hxu, *Huu, *hxx, *dHu, *hxe0, *dX, *dU, *lqr, *xt, *ut, *Jt;
    OcSolveState st;
    int64_t bytes;
    OcSolveWs(void* base, int B, int T, int K) {
        constexpr int n = Mdl::NX, m = Mdl::NU;
        char* p = (char*)base;
        int64_t off = 0;
        auto take = [&](int64_t count, int64_t elem) { void* r = p ? p + off : nullptr; off += (count * elem + 255) / 256 * 256; return r; };
        const int64_t BT = (int64_t)B * T;
        lam_eff = (double*)take(BT * n, 8); F = (double*)take(BT * n * n, 8); G = (double*)take(BT * n * m, 8);
        Hxx = (double*)take(BT * n * n, 8); Hxu = (double*)take(BT * n * m, 8); Huu = (double*)take(BT * m * m, 8);
        hxx = (double*)take((int64_t)B * n * n, 8); dHu = (double*)take(BT * m, 8); hxe0 = (double*)take((int64_t)B * n, 8);
        dX = (double*)take((int64_t)B * (T + 1) * n, 8); dU = (double*)take(BT * m, 8); lqr = (double*)take(BT * (n * m + m), 8);
        xt = (double*)take((int64_t)B * K * (T + 1) * n, 8); ut = (double*)take((int64_t)B * K * T * m, 8); Jt = (double*)take((int64_t)B * K, 8);
        st.J = (double*)take(B, 8); st.mu = (double*)take(B, 8); st.gnorm = (double*)take(B, 8);
        st.newton = (int32_t*)take(B, 4); st.converged = (int32_t*)take(B, 4); st.lqr_status = (int32_t*)take(B, 4); st.counters = (int32_t*)take(2, 4);
        bytes = off;
    }
};

template <class Mdl>
int oc_solve(int B, int T, const double* x0, const double* th, int tb, double* u, double* x, double* lam, double* cost, double* grad_norm,
             int32_t* converged, double* gains, const pdp_oc_solve_opts* op, int* iterations, void* ws, int64_t wsb, void* stv) {
    if constexpr (Mdl::KIND == PDP_KIND_OC && lqr_generic_in_lds(Mdl::NX, Mdl::NU, 1)) {      // beyond n = 16 / m = 4 the LQ step runs on the size-generic kernel (working set in LDS: n up to ~75)
        constexpr int n = Mdl::NX, m = Mdl::NU;
        if (B <= 0 || T <= 0 || !x0 || !th || !u || !x || !lam || !op || !ws) return PDP_E_ARG;
        const int K = op->ls_trials > 0 ? op->ls_trials : 10, every = op->check_every > 0 ? op->check_every : 4;
        OcSolveWs<Mdl> w(ws, B, T, K);
        if (wsb < w.bytes) return PDP_E_ARG;
        hipStream_t st = S(stv);
        const int nchunk = (T + auxsys_chunk<Mdl>() - 1) / auxsys_chunk<Mdl>();
        const dim3 gaux((unsigned)((int64_t)B * (nchunk + 1))), gB((B + 63) / 64), gBK((B * K + 63) / 64);
        clear_stale_error();
        (void)hipMemsetAsync(w.hxe0, 0, sizeof(double) * B * n, st);
        (void)hipMemsetAsync(w.st.mu, 0, sizeof(double) * B, st);
        (void)hipMemsetAsync(w.st.newton, 0, sizeof(int32_t) * B, st);
        (void)hipMemsetAsync(w.st.counters, 0, sizeof(int32_t) * 2, st);
        enqueue(oc_rollout_kernel<Mdl>, gB, dim3(64), 0, st, B, T, x0, u, th, tb, x, w.st.J);
        // LQ sub-problem for (dx, du): the LQR.lqrSolver kernel with p = 1, Hue := H_u, E = Hxe = 0 (PDP.py:557-608)
        pdp_lqr_problem pr{};
        pr.B = B; pr.T = T; pr.n = n; pr.m = m; pr.p = 1;
        pr.F = {w.F, (int64_t)T * n * n, n * n}; pr.G = {w.G, (int64_t)T * n * m, n * m}; pr.Hxx = {w.Hxx, (int64_t)T * n * n, n * n};
        pr.Hxu = {w.Hxu, (int64_t)T * n * m, n * m}; pr.Huu = {w.Huu, (int64_t)T * m * m, m * m}; pr.Hue = {w.dHu, (int64_t)T * m, m};
        pr.hxx = {w.hxx, n * n, 0}; pr.hxe = {w.hxe0, n, 0};
        double* const none = nullptr;
        auto lq = [&]() {
            if constexpr (n <= 4 && m <= 4)       // small systems: four trajectories per wavefront (pdp_riccati_small.h; its tile rows hold m <= 4 controls)
                enqueue(lqr_solve_small_kernel<m>, dim3((B + 3) / 4), dim3(64), 0, st, pr, w.dX, w.dU, none, w.st.lqr_status, w.lqr, none);
            else if constexpr (n <= 16 && m <= 4)
                enqueue(lqr_solve_kernel<m, 1>, dim3(B), dim3(64), 0, st, pr, w.dX, w.dU, none, w.st.lqr_status, w.lqr, none);
            else
                enqueue(lqr_solve_generic_kernel<false>, dim3(B), dim3(64), sizeof(double) * lqr_generic_lds_doubles(n, m, 1), st, pr, w.dX, w.dU, none, w.st.lqr_status, w.lqr,
                        none, none);
        };
        pdp_oc_auxsys only_hu{}, hess{};
        only_hu.dHu = w.dHu;
        hess.dynF = w.F; hess.dynG = w.G; hess.Hxx = w.Hxx; hess.Hxu = w.Hxu; hess.Huu = w.Huu; hess.hxx = w.hxx; hess.Huu_damp = w.st.mu;
        auto costate = [&]() { enqueue(oc_costate_kernel<Mdl>, gB, dim3(64), 0, st, B, T, x, u, th, tb, lam); };
        auto auxsys = [&](const double* l, const pdp_oc_auxsys& o) { enqueue(oc_auxsys_kernel<Mdl>, gaux, dim3(64), 0, st, B, T, x, u, l, th, tb, o); };
        int it = 0, last_nconv = 0, last_gain = 0, nconv = 0;
        for (it = 0; it < op->max_iter; ++it) {
            costate();
            auxsys(lam, only_hu);
            enqueue(oc_newton_prepare_kernel<Mdl>, dim3(B), dim3(64), 0, st, B, T, it, op->tol, op->newton_switch, u, w.dHu, lam, w.lam_eff, w.st);
            if (it % every == 0 || op->print_level > 0) {                 // poll the number of converged samples (synchronises the stream)
                int32_t c = 0;
                if (hipMemcpyAsync(&c, &w.st.counters[it & 1], sizeof(c), hipMemcpyDeviceToHost, st) != hipSuccess) return PDP_E_LAUNCH;
                if (hipStreamSynchronize(st) != hipSuccess) { (void)launched(); return PDP_E_LAUNCH; }       // (launched(): the error text)
                nconv = c;
                if (op->print_level > 0) fprintf(stderr, "  pdp_oc_solve iter %3d  converged %d/%d\n", it, nconv, B);
                if (nconv == B) break;
                // stragglers: most of the batch done and nothing new for a while -> stop, the caller re-solves the rest from a neighbour
                if (nconv > last_nconv) { last_nconv = nconv; last_gain = it; }
                else if (op->straggler_patience > 0 && nconv >= 0.9 * B && it - last_gain >= op->straggler_patience) break;
            }
            auxsys(w.lam_eff, hess);
            lq();
            enqueue(oc_linesearch_kernel<Mdl>, gBK, dim3(64), 0, st, B, T, K, x0, u, x, w.lqr, th, tb, w.xt, w.ut, w.Jt);
            enqueue(oc_ls_select_kernel<Mdl>, dim3(B), dim3(64), 0, st, B, T, K, w.dHu, w.dU, w.xt, w.ut, w.Jt, x, u, w.st);
        }
        if (it == op->max_iter) costate();
        if (gains) {       // time-varying LQR feedback around the final trajectory (full Hamiltonian Hessians, no damping)
            hess.Huu_damp = nullptr;
            auxsys(lam, only_hu);
            auxsys(lam, hess);
            lq();
            (void)hipMemcpyAsync(gains, w.lqr, sizeof(double) * (int64_t)B * T * (n * m + m), hipMemcpyDeviceToDevice, st);
        }
        if (cost) (void)hipMemcpyAsync(cost, w.st.J, sizeof(double) * B, hipMemcpyDeviceToDevice, st);
        if (grad_norm) (void)hipMemcpyAsync(grad_norm, w.st.gnorm, sizeof(double) * B, hipMemcpyDeviceToDevice, st);
        if (converged) (void)hipMemcpyAsync(converged, w.st.converged, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, st);
        if (iterations) *iterations = it;
        return launched();
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}

// Multiple-shooting solver variants (environment PDP_MS_VARIANT overrides): 2 = runner / evaluator wave pair per trajectory
// (pdp_ocsolve2_kernels.h), the default wherever its LDS layout fits; 1 = one wavefront per trajectory (pdp_ocsolve_kernels.h).
template <class Mdl>
int64_t oc_solve_ms_ws_bytes(int B, int T, int max_iter) {
    if constexpr (Mdl::KIND == PDP_KIND_OC) {
        const int64_t a = (int64_t)B * MsLayout<Mdl>::ws_doubles(T, max_iter < 0 ? 0 : max_iter) * (int64_t)sizeof(double);
        const int64_t c = ms2_ws_bytes<Mdl>(B, T, max_iter);
        return a > c ? a : c;                       // either variant may serve the call
    } else return 0;
}
template <class Mdl>
int oc_solve_ms(int B, int T, const double* x0, const double* th, int tb, double* x, double* u, double* lam, double* cost, double* resid,
                int32_t* converged, int32_t* iterations, int32_t* status, double* gains, double* iter_log, const pdp_oc_ms_opts* op, void* ws, int64_t wsb,
                void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_OC && Mdl::NX <= 16 && Mdl::NU <= 4) {
        if (B <= 0 || T <= 0 || !x0 || !th || !x || !u || !lam || !op || !ws) return PDP_E_ARG;
        if (op->max_iter < 0 || wsb < oc_solve_ms_ws_bytes<Mdl>(B, T, op->max_iter)) return PDP_E_ARG;
        const bool needs_pair = (op->flags & PDP_MS_FROM_CONTROLS) != 0;       // (the one-wave kernel has no restoration pass to start from)
        if (needs_pair && !(op->flags & PDP_MS_WARM)) return PDP_E_ARG;
        const bool watchdog = (op->flags & PDP_MS_WITH_WATCHDOG) != 0;
        const bool predict = (op->flags & PDP_MS_PREDICT) != 0;
        if ((op->flags & PDP_MS_PREDICT_PRIMAL) && (!predict || !op->predict_record)) return PDP_E_ARG;
        if (predict && (!(op->flags & PDP_MS_WARM) || needs_pair || !op->dtheta || (!op->predict_record && (!op->dxdp || !op->dudp)))) return PDP_E_ARG;
        // PDP_MS_PREDICT is applied by the runner / evaluator kernel while it loads the point (dx parked in its LDS pool); where that kernel does not run, or the
        // horizon outgrows the pool, the prediction is a launch of its own in front of the solve (pdp_oc_predict_batched, in place on x, u, lam)
        pdp_oc_ms_opts op1 = *op;
        auto predict_first = [&]() -> int {
            if (!predict) return 0;
            op1.flags &= ~PDP_MS_PREDICT;
            if constexpr (Mdl::NU + Mdl::NP <= 16) {
                if (op->predict_record)
                    return oc_predict_rec<Mdl>(B, T, op->dtheta, op->dtheta_bstride, op->predict_record, x, u, (op->flags & PDP_MS_PREDICT_PRIMAL) ? nullptr : lam, st);
                return oc_predict<Mdl>(B, T, op->dtheta, op->dtheta_bstride, op->dxdp, op->dudp, op->riccati, x, u, op->riccati ? lam : nullptr, st);
            } else return PDP_E_SIZE;
        };
        auto run = [&](auto kern, int wgs, int threads, size_t lds_bytes) {          // (either kernel; with the options as they stand at the launch)
            return launch(kern, dim3(wgs), dim3(threads), lds_bytes, S(st), B, T, op1, x0, th, tb, x, u, lam, cost, resid, converged, iterations, status, gains,
                          op1.log_rows > 0 ? iter_log : (double*)nullptr, (double*)ws);
        };
        static const int variant = env_int("PDP_MS_VARIANT", 2);
        if constexpr (ms2_ok<Mdl>()) {
            if (variant == 2 || needs_pair) {
                if (predict && !op->predict_record && !Ms2Layout<Mdl>::predict_fits(T)) { const int rc = predict_first(); if (rc != 0) return rc; }      // (the record is staged block by block: any horizon)
                auto pair = [&](auto K, auto WD) {
                    return run(oc_solve_ms2_kernel<Mdl, K(), WD()>, (B + K() - 1) / K(), 128 * K(), K() * Ms2Layout<Mdl>::SLICE * sizeof(double));
                };
                // PDP_MS_WITH_WATCHDOG: the instantiations with the watchdog, one / two trajectories per workgroup whatever the batch (see the kernel's template line)
                const int cus = device_cu_count();
                if (watchdog) return with_int<1, 2>(traj_per_workgroup(B, cus, 2), [&](auto K) { return pair(K, std::true_type{}); });
                return with_int<1, 2, 4>(traj_per_workgroup(B, cus, 4), [&](auto K) { return pair(K, std::false_type{}); });
            }
        }
        if (needs_pair || watchdog) return PDP_E_SIZE;      // (only the runner / evaluator kernel restores, and only it has the watchdog)
        const size_t lds = ms_lds_bytes<Mdl>();
        if (lds > 160 * 1024) return PDP_E_SIZE;
        { const int rc = predict_first(); if (rc != 0) return rc; }
        return run(oc_solve_ms_kernel<Mdl>, B, 64, lds);
    } else { return Mdl::KIND == PDP_KIND_OC ? PDP_E_SIZE : PDP_E_MODE; }
}

// The MLP policy's shape, walked once for every entry point that asks about it (zeros for the other policy kinds).  Only the first GEN_MAXL layers are read
// (the length of pdp_policy.sizes): `beyond` already holds for a deeper network.
struct MlpShape {
    int layers;            // n_layers as given
    int64_t params;        // weights and biases: the length the parameter vector must have
    int out, widest;       // rows of the last layer (NX without layers); the widest layer
    int hidden;            // units of all layers but the last: the activations a reverse pass keeps per time step
    bool positive;         // every layer has at least one unit
    bool beyond;           // more than 8 layers or a layer wider than MLP_MAX_WIDTH: beyond the lane-local arrays of the lane-per-trajectory kernels
};
template <class Mdl>
MlpShape mlp_shape(const pdp_policy& pol) {
    MlpShape s{0, 0, Mdl::NX, 0, 0, true, false};
    if (pol.kind != PDP_POLICY_MLP) return s;
    s.layers = pol.n_layers;
    for (int k = 0; k < pol.n_layers && k < GEN_MAXL; ++k) {
        const int rows = pol.sizes[k];
        s.params += (int64_t)rows * s.out + rows;
        s.out = rows;
        s.widest = rows > s.widest ? rows : s.widest;
        if (k + 1 < pol.n_layers) s.hidden += rows;
        s.positive = s.positive && rows >= 1;
    }
    s.beyond = pol.n_layers > 8 || s.widest > MLP_MAX_WIDTH;
    return s;
}
template <class Mdl> bool cp_policy_args_ok(const pdp_policy* pol, int p);
template <class Mdl>
int cp_integrate(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* th, int tb, double* x, double* u, double* cost, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (B <= 0 || T <= 0 || !pol || !x0 || !th) return PDP_E_ARG;
        // (networks beyond the lane-local arrays of this lane-per-trajectory integrator: PDP_E_SIZE tells the caller to take pdp_cp_step_batched's size-generic kernel,
        // which rolls out as well - runtime.cp_integrate does)
        if (mlp_shape<Mdl>(*pol).beyond) return PDP_E_SIZE;
        return launch(cp_integrate_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, *pol, p, x0, th, tb, x, u, cost);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int cp_auxsys(int B, int T, const pdp_policy* pol, int p, const double* x, const double* u, const double* th, int tb, double* F, double* G,
              double* Ux, double* Ue, double* cx, double* cu, double* hx, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (B <= 0 || T <= 0 || !pol || !x || !u || !th) return PDP_E_ARG;
        const MlpShape net = mlp_shape<Mdl>(*pol);
        const bool wide = net.beyond;            // a network beyond the lane-local arrays of cp_auxsys_kernel: its Jacobians come from the wave-per-(b, t) kernel
        const int64_t n = (int64_t)B * (T + 1);
        clear_stale_error();
        enqueue(cp_auxsys_kernel<Mdl>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, S(st), B, T, *pol, p, x, u, th, tb, F, G, wide ? nullptr : Ux, wide ? nullptr : Ue, cx, cu, hx);
        if (wide && Ux && Ue) {
            if (!cp_policy_args_ok<Mdl>(pol, p)) return PDP_E_ARG;
            const int sum_in = Mdl::NX + net.hidden, maxw = net.widest > Mdl::NX ? net.widest : Mdl::NX;
            const size_t lds = sizeof(double) * ((size_t)sum_in + 2 * (size_t)maxw + 8);
            if (lds > 150 * 1024) return PDP_E_SIZE;           // (layer inputs of more than ~19 000 units in total)
            enqueue(cp_policy_jac_generic_kernel<Mdl::NX, Mdl::NU>, dim3((unsigned)((int64_t)B * T)), dim3(64), lds, S(st), B, T, *pol, p, x, th, tb, Ux, Ue, sum_in, maxw);
        }
        return launched();
    } else { return PDP_E_MODE; }
}
// Batches from which ControlPlanning.step with the Lagrange policy rolls out beforehand, one LANE per trajectory, and runs the sensitivity kernel on the given trajectories
// (cp_poly_rollout_lanes_kernel + cp_step_poly_kernel<.., GIVEN>): more than two trajectories per SIMD, like SysID.step.  PDP_CP_PREPASS=0 / 1 forces it off / on.
inline bool cp_prepass(int B) {
    static const int env = env_int("PDP_CP_PREPASS", -1);
    return env >= 0 ? env != 0 : B > 8 * device_cu_count();
}
// workspace of the pre-pass: x [B][T+1][NX] | u [B][T][NU] | h_x [B][NX]
template <class Mdl>
int64_t cp_prepass_ws_bytes(int B, int T) { return (int64_t)B * ((int64_t)(T + 1) * Mdl::NX + (int64_t)T * Mdl::NU + Mdl::NX) * (int64_t)sizeof(double); }
template <class Mdl, int NT>
int cp_step_given_launch(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* th, int tb, double* loss, double* grad, double* x, double* u,
                         double* ws, void* st) {
    constexpr int NX = Mdl::NX, NU = Mdl::NU, STRIDE = Mdl::PATH_NVAR | 1;
    const int np = pol->n_pivots;
    double* xw = x ? x : ws;                                                   // the API outputs double as the hand-over where the caller asked for them
    double* uw = u ? u : ws + (int64_t)B * (T + 1) * NX;
    double* hxw = ws + (int64_t)B * ((int64_t)(T + 1) * NX + (int64_t)T * NU);
    const size_t lds0 = sizeof(double) * ((size_t)T * np + (size_t)p * 64);
    if (lds0 > 150 * 1024) return PDP_E_SIZE;
    if (const int rc = launch(cp_poly_rollout_lanes_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), lds0, S(st), B, T, *pol, p, x0, th, tb, loss, xw, uw, hxw); rc != 0) return rc;
    static const int wgs_env = env_int("PDP_CP_GIVEN_WGS", 0);
    const int wgs = wgs_env > 0 ? wgs_env : 12;
    const int fixed = 1 + Mdl::PATH_NCONST + T * np + NX + 8 + 64 + (NX > NU ? NX : NU);
    int rows = (160 * 1024 / 8 / wgs - 64 - fixed) / STRIDE;
    rows = rows > Mdl::CHUNK ? Mdl::CHUNK : (rows < 4 ? (Mdl::CHUNK < 4 ? Mdl::CHUNK : 4) : rows);
    const size_t lds = sizeof(double) * ((size_t)fixed + (size_t)rows * STRIDE);
    if (lds > 150 * 1024) return PDP_E_SIZE;
    return launch(cp_step_poly_kernel<Mdl, NT, true>, dim3(B, 1), dim3(64), lds, S(st), B, T, *pol, p, x0, th, tb, loss, grad, x, u, rows, (const double*)xw,
                  (const double*)uw, (const double*)hxw);
}
// Lagrange-policy kernel variants (environment PDP_CP_POLY_VARIANT overrides): 2 = rollout wave + sensitivity wave per trajectory (pdp_cp_pair_kernels.h) for
// batches above one trajectory per CU, the default; 3 = the pair for every batch; 1 = one wavefront per trajectory and group of parameter tiles (cp_step_poly_kernel)
inline int cp_poly_variant() { static const int v = env_int("PDP_CP_POLY_VARIANT", 2); return v; }
// MLP kernel variants (environment PDP_CP_MLP_VARIANT overrides): 2 = network in registers (pdp_cp_mlp_kernels.h), the default for networks of at
// most 4 layers of width <= 16 - four trajectories per wavefront on the 4-block MFMA for shared parameters from two trajectories per CU on, one trajectory per
// wavefront otherwise; 3 = one trajectory per wavefront for every batch (round 4's route); 4 = four per wavefront for every batch; 1 = the general adjoint kernel
// (any policy up to 8 layers x 32 units)
inline int cp_mlp_variant() { static const int v = env_int("PDP_CP_MLP_VARIANT", 2); return v; }
// ---- the size-generic route of ControlPlanning.step (csrc/pdp_cp_generic_kernels.h): whatever the tuned kernels below do not take
template <class Mdl>
bool cp_policy_args_ok(const pdp_policy* pol, int p) {        // the parameter vector has the length the policy implies
    if (pol->kind == PDP_POLICY_POLY) return pol->n_pivots >= 1 && pol->n_pivots <= 16 && p == pol->n_pivots * Mdl::NU;
    if (pol->kind == PDP_POLICY_TABLE) return pol->n_basis >= 1 && pol->table != nullptr && p == pol->n_basis * Mdl::NU;
    const MlpShape net = mlp_shape<Mdl>(*pol);
    return pol->kind == PDP_POLICY_MLP && net.layers >= 1 && net.layers <= GEN_MAXL && net.positive && net.params == p && net.out == Mdl::NU;
}
template <class Mdl>
bool cp_needs_generic(const pdp_policy* pol, int p) {
    if (Mdl::NX > 16 || Mdl::NU > 4) return true;                                  // beyond one tile per matrix
    if (pol->kind == PDP_POLICY_TABLE) return true;
    return pol->kind == PDP_POLICY_MLP && (p > 512 || mlp_shape<Mdl>(*pol).beyond);
}
static int cp_generic_wide_bytes() { static const int v = env_int("PDP_CP_GENERIC_WIDE_BYTES", 96 * 1024); return v; }
template <class Mdl>
int cp_step_generic(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* th, int tb, double* loss, double* grad, double* x, double* u,
                    void* ws, int64_t wsb, void* st) {
    if (!cp_policy_args_ok<Mdl>(pol, p)) return PDP_E_ARG;
    if (Mdl::NX > 64 || Mdl::NU > 64) return PDP_E_SIZE;          // the size-generic adjoint kernel holds one Jacobian column per lane
    const CpGenLayout L = cp_generic_layout<Mdl>(*pol, T, x != nullptr, u != nullptr, cp_generic_wide_bytes());
    if (L.rows < 1 || (size_t)L.lds_total * sizeof(double) > 160 * 1024) return PDP_E_SIZE;       // (a model whose single Jacobian row exceeds the LDS: not a policy size)
    if (L.ws_per_traj > 0 && (!ws || wsb < (int64_t)B * L.ws_per_traj * (int64_t)sizeof(double))) return PDP_E_ARG;
    return with_bool(pol->kind == PDP_POLICY_MLP, [&](auto MLPK) {
        return launch(cp_step_generic_kernel<Mdl, MLPK()>, dim3(B), dim3(64), sizeof(double) * (size_t)L.lds_total, S(st), B, T, *pol, p, x0, th, tb, loss, grad, x, u, (double*)ws, L);
    });
}
template <class Mdl>
int64_t cp_step_ws_bytes(int B, int T, const pdp_policy* pol, int p) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (pol && cp_needs_generic<Mdl>(pol, p)) {
            if (!cp_policy_args_ok<Mdl>(pol, p)) return 0;
            return (int64_t)B * cp_generic_layout<Mdl>(*pol, T, false, false, cp_generic_wide_bytes()).ws_per_traj * (int64_t)sizeof(double);
        }
        if (pol && pol->kind == PDP_POLICY_POLY && p <= 64 && cp_prepass(B)) return cp_prepass_ws_bytes<Mdl>(B, T);
        if (!pol || pol->kind != PDP_POLICY_MLP || pol->n_layers < 1 || pol->n_layers > 8) return 0;
        if constexpr (Mdl::NX > 16 || Mdl::NU > 4) return 0; else {
        int64_t need = 0;
        if (cp_mlp16_ok<Mdl>(*pol)) {
            need = (int64_t)B * T * 64 * (int64_t)sizeof(double);                                // register kernel: one double per lane and time step
            const int64_t n4 = cp_mlp4t_ws_doubles<Mdl>(B, T) * (int64_t)sizeof(double);          // four-trajectory kernel: activations in D layout + the trajectories
            need = n4 > need ? n4 : need;
        }
        bool offload; int rows;
        cp_adjoint_plan<Mdl>(*pol, p, T, B, device_cu_count(), true, offload, rows);
        if (offload) {
            const int64_t a = (int64_t)B * T * mlp_shape<Mdl>(*pol).hidden * (int64_t)sizeof(double);
            need = a > need ? a : need;
        }
        return need;
        }
    } else { return 0; }
}
template <class Mdl>
int cp_step(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* th, int tb, double* loss, double* grad, double* x, double* u,
            void* ws, int64_t wsb, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (B <= 0 || T <= 0 || !pol || !x0 || !th || !loss || !grad) return PDP_E_ARG;
        if (cp_needs_generic<Mdl>(pol, p)) return cp_step_generic<Mdl>(B, T, pol, p, x0, th, tb, loss, grad, x, u, ws, wsb, st);       // (every call of a model beyond one tile per matrix)
        if constexpr (Mdl::NX <= 16 && Mdl::NU <= 4) {
        const int cus = device_cu_count();
        if (pol->kind == PDP_POLICY_MLP || p > 64) {          // adjoint (reverse-mode) kernel: MLP policy, or many Lagrange pivots
            if (p > 512) return PDP_E_SIZE;
            if (pol->kind == PDP_POLICY_MLP) {
                const MlpShape net = mlp_shape<Mdl>(*pol);
                if (net.layers < 1 || Mdl::NX > MLP_MAX_WIDTH || net.beyond || !net.positive) return PDP_E_SIZE;
                if (net.params != p || net.out != Mdl::NU) return PDP_E_ARG;
            } else if (p != pol->n_pivots * Mdl::NU || pol->n_pivots > 16) return PDP_E_ARG;
            // shared parameters (the reference's case: one policy for every initial state): four trajectories per wavefront on the 4-block MFMA (cp_step_mlp4t_kernel)
            // - from two trajectories per CU on (below that a wavefront per trajectory has a SIMD to itself and the same latency per step: measured 0.252 / 0.257 / 0.267 ms
            // against 0.272 for B = 64 / 256 / 512, probes/mlp4t_timing.py); PDP_CP_MLP_VARIANT=4 takes it for every batch (tests)
            if (pol->kind == PDP_POLICY_MLP && ((cp_mlp_variant() == 2 && B > 2 * cus) || cp_mlp_variant() == 4) && tb == 0 && cp_mlp16_ok<Mdl>(*pol) &&
                ws != nullptr && wsb >= cp_mlp4t_ws_doubles<Mdl>(B, T) * (int64_t)sizeof(double)) {
                const size_t lds4 = sizeof(double) * (size_t)cp_mlp4t_layout<Mdl>().total;
                return with_int<1, 2, 3, 4>(pol->n_layers, [&](auto NL) {
                    return launch(cp_step_mlp4t_kernel<Mdl, NL()>, dim3((B + 3) / 4), dim3(64), lds4, S(st), B, T, *pol, p, x0, th, loss, grad, x, u, (double*)ws);
                });
            }
            // PDP_CP_MLP_VARIANT=3: the one-trajectory register kernel for shared parameters as well (what round 4 ran; per-sample parameters always take it)
            if (pol->kind == PDP_POLICY_MLP && (cp_mlp_variant() >= 2) && cp_mlp16_ok<Mdl>(*pol) && ws != nullptr && wsb >= (int64_t)B * T * 64 * (int64_t)sizeof(double)) {
                // batches beyond one trajectory per SIMD: rows sized for eight workgroups per CU, i.e. two wavefronts per SIMD that fill each other's gaps (PDP_CP_MLP_LDS_KB overrides)
                static const int kb_env = env_int("PDP_CP_MLP_LDS_KB", 0);
                const int rows16 = cp_mlp16_rows<Mdl>(T, kb_env > 0 ? kb_env : (B > 4 * cus ? 20 : 40));
                const size_t lds16 = sizeof(double) * (size_t)cp_mlp16_layout<Mdl>(T, rows16).total;
                if (rows16 >= 1 && lds16 <= 160 * 1024)
                    return launch(cp_step_mlp16_kernel<Mdl>, dim3(B), dim3(64), lds16, S(st), B, T, *pol, p, x0, th, tb, loss, grad, x, u, (double*)ws, rows16);
            }
            bool offload; int rows;
            cp_adjoint_plan<Mdl>(*pol, p, T, B, cus, ws != nullptr && wsb >= cp_step_ws_bytes<Mdl>(B, T, pol, p), offload, rows);
            const size_t lds = sizeof(double) * (size_t)cp_adjoint_layout<Mdl>(*pol, p, T, offload, rows).total;
            if (lds > 160 * 1024) return PDP_E_SIZE;
            return launch(cp_step_adjoint_kernel<Mdl>, dim3(B), dim3(64), lds, S(st), B, T, *pol, p, x0, th, tb, loss, grad, x, u, offload ? (double*)ws : (double*)nullptr, rows);
        }
        if (p != pol->n_pivots * Mdl::NU || pol->n_pivots > 16) return PDP_E_ARG;
        const int nt = (p + 15) / 16;
        if (nt > 4) return PDP_E_SIZE;
        if (ws && cp_prepass(B) && wsb >= cp_prepass_ws_bytes<Mdl>(B, T))        // several trajectories per SIMD: rollout beforehand, one lane per trajectory
            return with_int<1, 2, 3, 4>(nt, [&](auto NT) { return cp_step_given_launch<Mdl, NT()>(B, T, pol, p, x0, th, tb, loss, grad, x, u, (double*)ws, st); });
        // rollout wave + sensitivity wave per trajectory (pdp_cp_pair_kernels.h) once the batch exceeds one trajectory per CU; below that the one-wave kernel with its
        // parameter tiles spread over grid.y does as well (profiles/r03_pair_pipeline.txt).  PDP_CP_POLY_VARIANT=3 takes the pair for every batch (tests)
        if ((cp_poly_variant() == 2 && B > cus) || cp_poly_variant() == 3) {
            const int slice = cp_pair_slice<Mdl>(T, pol->n_pivots), tpw = traj_per_workgroup(B, cus, 4);
            if ((size_t)slice * tpw * sizeof(double) <= 160 * 1024) {
                // tiles spread over several pairs only while whole CUs would idle (measured: C4 shard, 0.090 ms against 0.111 with twice as many pairs)
                const TileSplit sp = split_tiles(nt, (int64_t)2 * cus / B);
                return with_int<1, 2, 3, 4>(sp.per, [&](auto NT) {
                    return with_int<1, 2, 4>(tpw, [&](auto K) {
                        return launch(cp_step_poly2_kernel<Mdl, NT(), K()>, dim3((B + K() - 1) / K(), sp.gy), dim3(128 * K()), slice * K() * sizeof(double), S(st), B, T, *pol, p,
                                      x0, th, tb, loss, grad, x, u, slice);
                    });
                });
            }
        }
        // a batch that leaves SIMDs idle (one wavefront per trajectory, 4 SIMDs per CU) spreads the parameter tiles of a trajectory
        // over several wavefronts: each repeats the rollout and carries nt / gy of the sensitivity tiles
        const TileSplit sp = split_tiles(nt, (int64_t)4 * cus / B);
        const size_t lds = sizeof(double) * (1 + Mdl::PATH_NCONST + Mdl::CHUNK * (Mdl::PATH_NVAR | 1) + (size_t)(T + 1) * Mdl::NX + (size_t)T * Mdl::NU +
                                             (size_t)T * pol->n_pivots + Mdl::NX + 8 + 64 + (Mdl::NX > Mdl::NU ? Mdl::NX : Mdl::NU));
        if (lds > 150 * 1024) return PDP_E_SIZE;
        return with_int<1, 2, 3, 4>(sp.per, [&](auto NT) {
            return launch(cp_step_poly_kernel<Mdl, NT()>, dim3(B, sp.gy), dim3(64), lds, S(st), B, T, *pol, p, x0, th, tb, loss, grad, x, u, 0, (const double*)nullptr,
                          (const double*)nullptr, (const double*)nullptr);
        });
        } else return PDP_E_SIZE;       // (not reached: cp_needs_generic holds for such a model)
    } else { return PDP_E_MODE; }
}

// pdp_cp_step_batched with PDP_POLICY_COTANGENT (include/pdp_hip.h): the adjoint sweep of pdp_cp_vjp_kernels.h on the rollout the struct names, and no rollout.  The
// kernel receives the pdp_policy by value with the bit cleared.  Every refusal comes before the launch.  Limits: those of cp_step_adjoint_kernel.
template <class Mdl>
int cp_vjp(int B, int T, const pdp_policy_cot* pc, int p, const double* th, int tb, const double* loss, double* grad, const double* x, const double* u, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (B <= 0 || T <= 0 || !th || loss || x || u || (!grad && !pc->grad_x0) || !pc->x || !pc->grad_x || !pc->grad_u) return PDP_E_ARG;
        pdp_policy pol = pc->pol;
        pol.kind &= ~PDP_POLICY_COTANGENT;
        if (pol.kind != PDP_POLICY_POLY && pol.kind != PDP_POLICY_MLP && pol.kind != PDP_POLICY_TABLE) return PDP_E_ARG;
        if constexpr (Mdl::NX <= 16 && Mdl::NU <= 4) {
            if (pol.kind == PDP_POLICY_TABLE) return PDP_E_SIZE;
            if (pol.kind == PDP_POLICY_MLP) {
                const MlpShape net = mlp_shape<Mdl>(pol);
                if (net.layers < 1 || !net.positive) return PDP_E_ARG;
                if (net.beyond) return PDP_E_SIZE;
                if (net.params != p || net.out != Mdl::NU) return PDP_E_ARG;
            } else if (pol.n_pivots < 1 || pol.n_pivots > 16 || p != pol.n_pivots * Mdl::NU) return PDP_E_ARG;
            if (p > 512) return PDP_E_SIZE;
            constexpr int rows = oc_x0_vjp_rows_of(CpVjpPool<Mdl>::STRIDE);
            const size_t lds = sizeof(double) * (size_t)cp_vjp_layout<Mdl>(p, rows).total;
            if (lds > 150 * 1024) return PDP_E_SIZE;
            return launch(cp_vjp_kernel<Mdl>, dim3(B), dim3(64), lds, S(st), B, T, pol, p, pc->x, th, tb, pc->grad_x, pc->grad_u, grad, pc->grad_x0, rows);
        } else { return PDP_E_SIZE; }
    } else { return PDP_E_MODE; }
}
// pdp_cp_step_batched with PDP_POLICY_TANGENT (include/pdp_hip.h): the tangent sweep of pdp_cp_jvp_kernels.h on the rollout and the controls the struct names, and no
// rollout.  As above: the pdp_policy by value with the bit cleared, every refusal before the launch, the limits of cp_step_adjoint_kernel.
template <class Mdl>
int cp_jvp(int B, int T, const pdp_policy_tan* pt, int p, const double* th, int tb, const double* loss, const double* grad, const double* x, const double* u, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_CP) {
        if (B <= 0 || T <= 0 || !th || loss || grad || x || u || (!pt->d_theta && !pt->d_x0) || !pt->x || !pt->u || !pt->d_x) return PDP_E_ARG;
        if (pt->d_theta && pt->d_theta_bstride != 0 && pt->d_theta_bstride != p) return PDP_E_ARG;
        pdp_policy pol = pt->pol;
        pol.kind &= ~PDP_POLICY_TANGENT;                                   // (with PDP_POLICY_COTANGENT beside it what is left is no policy kind)
        if (pol.kind != PDP_POLICY_POLY && pol.kind != PDP_POLICY_MLP && pol.kind != PDP_POLICY_TABLE) return PDP_E_ARG;
        if constexpr (Mdl::NX <= 16 && Mdl::NU <= 4) {
            if (pol.kind == PDP_POLICY_TABLE) return PDP_E_SIZE;
            if (pol.kind == PDP_POLICY_MLP) {
                const MlpShape net = mlp_shape<Mdl>(pol);
                if (net.layers < 1 || !net.positive) return PDP_E_ARG;
                if (net.beyond) return PDP_E_SIZE;
                if (net.params != p || net.out != Mdl::NU) return PDP_E_ARG;
            } else if (pol.n_pivots < 1 || pol.n_pivots > 16 || p != pol.n_pivots * Mdl::NU) return PDP_E_ARG;
            if (p > 512) return PDP_E_SIZE;
            constexpr int rows = oc_x0_vjp_rows_of(CpJvpPool<Mdl>::STRIDE);
            const size_t lds = sizeof(double) * (size_t)cp_jvp_layout<Mdl>(p, rows).total;
            if (lds > 150 * 1024) return PDP_E_SIZE;
            return launch(cp_jvp_kernel<Mdl>, dim3(B), dim3(64), lds, S(st), B, T, pol, p, pt->x, pt->u, th, tb, pt->d_theta, pt->d_theta_bstride, pt->d_x0, pt->d_x,
                          pt->d_u, rows);
        } else { return PDP_E_SIZE; }
    } else { return PDP_E_MODE; }
}
// the entry points that serve neither a pdp_policy_cot nor a pdp_policy_tan
inline bool cp_cot(const pdp_policy* pol) { return pol && (pol->kind & (PDP_POLICY_COTANGENT | PDP_POLICY_TANGENT)) != 0; }
constexpr int cp_cot_refusal() { return PdpModel::KIND == PDP_KIND_CP ? PDP_E_ARG : PDP_E_MODE; }

template <class Mdl>
int sysid_integrate(int B, int T, const double* x0, const double* u, const double* th, int tb, double* x, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_SYSID) {
        if (B <= 0 || T <= 0 || !x0 || !u || !th || !x) return PDP_E_ARG;
        return launch(sysid_integrate_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, x0, (int)Mdl::NX, u, th, tb, x);
    } else { return PDP_E_MODE; }
}
template <class Mdl>
int sysid_auxsys(int B, int T, const double* x, const double* u, const double* th, int tb, double* F, double* E, void* st) {
    if constexpr (Mdl::KIND == PDP_KIND_SYSID) {
        if (B <= 0 || T <= 0 || !x || !u || !th) return PDP_E_ARG;
        const int64_t n = (int64_t)B * T;
        return launch(sysid_auxsys_kernel<Mdl>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, S(st), B, T, x, u, th, tb, F, E);
    } else { return PDP_E_MODE; }
}
// Batches from which SysID.step rolls the trajectories out beforehand, one LANE per trajectory (sysid_integrate_kernel into the caller's workspace), and runs the fused
// kernel on the given trajectories: more than two trajectories per SIMD (profiles/r04_rollout_prepass.txt).  PDP_SYSID_PREPASS=0 / 1 forces it off / on.
inline bool sysid_prepass(int B) {
    static const int env = env_int("PDP_SYSID_PREPASS", -1);
    return env >= 0 ? env != 0 : B > 8 * device_cu_count();
}
// workgroups per CU that the pool rows of the given-trajectory kernel are sized for (sysid_rows_given): three wavefronts per SIMD at the plain instantiation's 162
// VGPRs; the Gauss-Newton instantiations carry one more accumulator tile (quadrotor: 174 / 176 VGPRs, no spill) and get two per SIMD - their rows are sized for the
// eight workgroups that are resident
template <int MODE> constexpr int SYSID_GIVEN_WGS = MODE == PDP_SYSID_PLAIN ? 12 : 8;
template <class Mdl>
int64_t sysid_step_ws_bytes(int B, int T) {
    if constexpr (Mdl::KIND == PDP_KIND_SYSID) return sysid_prepass(B) ? (int64_t)B * (T + 1) * Mdl::NX * (int64_t)sizeof(double) : 0;
    else return 0;
}
// MODE (PDP_SYSID_PLAIN / PDP_SYSID_GN / PDP_SYSID_GN_MISS): the instantiation of the fused kernels.  The Gauss-Newton modes write the packed row grad | loss | G through
// `grad`, start the rollouts from x0 [B][n] (NULL: x_obs[:, 0]) - in the kernels through their trailing argument, in the pre-pass through its pointer and stride - and
// exist for p <= 16.  PDP_SYSID_GN_INI / PDP_SYSID_GN_INI_MISS: the Gauss-Newton modes with the components of x0 that `ini_mask` names as further unknowns (the
// kernels' second trailing argument; the row is grad | loss | G over W = p + popcount(ini_mask) <= 16 unknowns).  PDP_SYSID_GN_W / PDP_SYSID_GN_W_INI: weighted and
// Huber-robust least squares on PDP_SYSID_GN / PDP_SYSID_GN_INI (`wls`, the kernels' last trailing argument; NX more words per pool row and behind dlT, and the
// Gauss-Newton modes' eight workgroups per CU in the given-trajectory kernel).  The LDS slice and the trailing pack follow from MODE: SysidLayout, SysidArgs.  Same dispatch, thresholds and switches in every mode.
template <class Mdl, int MODE = PDP_SYSID_PLAIN>
int sysid_step(int B, int T, const double* u, const double* xobs, const double* th, int tb, double* loss, double* grad, void* ws, int64_t wsb, void* st,
               const double* x0 = nullptr, [[maybe_unused]] unsigned ini_mask = 0, [[maybe_unused]] SysidWls wls = {}) {
    constexpr bool INI = SysidMode<MODE, 1>::INI;
    if constexpr (Mdl::KIND == PDP_KIND_SYSID && Mdl::NX <= 16 && Mdl::NP <= (MODE == PDP_SYSID_PLAIN ? 64 : (INI ? 15 : 16))) {
        if (B <= 0 || T <= 0 || !u || !xobs || !th || !loss || !grad) return PDP_E_ARG;
        if constexpr (INI) { if (Mdl::NP + __builtin_popcount(ini_mask) > 16) return PDP_E_SIZE; }
        const double* xgiven = nullptr;
        if (ws && sysid_prepass(B)) {           // (no workspace: the kernel rolls out itself, whatever the batch)
            if (wsb < sysid_step_ws_bytes<Mdl>(B, T)) return PDP_E_ARG;
            if (const int rc = launch(sysid_integrate_kernel<Mdl>, dim3((B + 63) / 64), dim3(64), 0, S(st), B, T, x0 ? x0 : xobs,
                                      (int)(x0 ? Mdl::NX : (T + 1) * Mdl::NX), u, th, tb, (double*)ws); rc != 0)
                return rc;
            xgiven = (const double*)ws;
        }
        constexpr int NT = (Mdl::NP + 15) / 16;
        static const int rows_env = env_int("PDP_SYSID_ROWS", 0), wgs_env = env_int("PDP_SYSID_GIVEN_WGS", 0);
        const int cus = device_cu_count();
        const int rows = rows_env > 0 ? (rows_env < Mdl::CHUNK ? rows_env : Mdl::CHUNK)
                         : (xgiven ? sysid_rows_given<Mdl, MODE>(T, wgs_env > 0 ? wgs_env : SYSID_GIVEN_WGS<MODE>) : sysid_rows<Mdl, MODE>(B, T, cus));
        const size_t lds = sizeof(double) * (size_t)sysid_slice<Mdl, MODE>(T, rows, xgiven != nullptr);
        if (lds > 150 * 1024) return PDP_E_SIZE;
        // the kernels' trailing arguments, a tuple whose TYPE is fixed by MODE (SysidArgs): the kernels' `Ini...` is spelled from its element types, never from a call's arguments
        const SysidArgs<MODE> trailing = sysid_args<MODE>(x0, ini_mask, wls);
        // PDP_SYSID_VARIANT: 2 = rollout wave + sensitivity wave per trajectory (sysid_step2_kernel), the default; 1 = one wavefront per trajectory
        static const int variant = env_int("PDP_SYSID_VARIANT", 2);
        return std::apply([&](auto... extra) {
            // the pair pays while SIMDs would idle (B = 256, T = 200: 0.105 -> 0.072 ms); once every SIMD has a trajectory the two waves only share what one had
            // (B = 1024: 0.0667 against 0.0685 ms, profiles/r03_pair_pipeline.txt) - the one-wave kernel stays for those batches
            if (variant == 2 && B <= 2 * cus && !xgiven) {
                const int slice = sysid_slice<Mdl, MODE>(T, Mdl::CHUNK, false), tpw = traj_per_workgroup(B, cus, 2);
                if (slice * tpw * (int)sizeof(double) <= 160 * 1024)
                    return with_int<1, 2>(tpw, [&](auto K) {
                        return launch(sysid_step2_kernel<Mdl, NT, K(), MODE, decltype(extra)...>, dim3((B + K() - 1) / K()), dim3(128 * K()), slice * K() * sizeof(double),
                                      S(st), B, T, u, xobs, th, tb, loss, grad, slice, extra...);
                    });
            }
            return with_bool(xgiven != nullptr, [&](auto GIVEN) {
                return launch(sysid_step_kernel<Mdl, NT, GIVEN(), MODE, decltype(extra)...>, dim3(B), dim3(64), lds, S(st), B, T, u, xobs, th, tb, loss, grad, rows, xgiven,
                              extra...);
            });
        }, trailing);
    } else { return Mdl::KIND == PDP_KIND_SYSID ? PDP_E_SIZE : PDP_E_MODE; }
}

// The plan of a SysID sweep launch (pdp_sweep_pool.h) for a batch of B: the pool rows and the bytes of dynamic LDS, or in `rows` the error - PDP_E_MODE for another
// model kind, PDP_E_SIZE where the kernel is not built for the model (FITS, known at compile time: `ok` tells the caller whether to name the kernel at all) or its
// block exceeds 150 KB.  The argument checks come before it, whatever the model.
template <bool OK> struct SweepPlan { static constexpr bool ok = OK; int rows; size_t lds; };
template <class Mdl, template <class> class PoolOf, bool FITS>
auto sweep_plan(int B) {
    if constexpr (Mdl::KIND != PDP_KIND_SYSID) return SweepPlan<false>{PDP_E_MODE, 0};
    else if constexpr (!FITS) return SweepPlan<false>{PDP_E_SIZE, 0};
    else {
        const int rows = sysid_vjp_rows_of(B, device_cu_count(), PoolOf<Mdl>::STRIDE, Mdl::CHUNK);
        const size_t lds = sizeof(double) * (size_t)PoolOf<Mdl>::slice(rows);
        return lds > 150 * 1024 ? SweepPlan<true>{PDP_E_SIZE, 0} : SweepPlan<true>{rows, lds};
    }
}
// the kernels exist for n <= 64 and eight slots of 64 columns per lane: p <= 512 parameters, p + m <= 512 where a lane also owns the columns of G
template <class Mdl> constexpr bool sweep_fits_p = Mdl::NX <= 64 && Mdl::NP <= 512;
template <class Mdl> constexpr bool sweep_fits_pm = Mdl::NX <= 64 && Mdl::NP + Mdl::NU <= 512;

// The rollout's vector-Jacobian product (pdp_sysid_rollout_vjp_batched, include/pdp_hip_sysid_vjp.h): one launch of sysid_vjp_kernel on the given trajectory.
template <class Mdl>
int sysid_rollout_vjp(int B, int T, const double* x, const double* u, const double* th, int tb, const double* gx, double* grad_theta, double* grad_x0, void* st) {
    if (B <= 0 || T <= 0 || !x || !u || !th || !gx || (!grad_theta && !grad_x0) || (tb != 0 && tb < Mdl::NP)) return PDP_E_ARG;
    const auto pl = sweep_plan<Mdl, SysidVjpPool, sweep_fits_p<Mdl>>(B);
    if constexpr (!pl.ok) return pl.rows;
    else return pl.rows < 0 ? pl.rows : launch(sysid_vjp_kernel<Mdl>, dim3(B), dim3(64), pl.lds, S(st), B, T, x, u, th, tb, gx, grad_theta, grad_x0, pl.rows);
}

// ... and with the gradient with respect to the inputs (pdp_sysid_rollout_vjp_u_batched, include/pdp_hip_sysid_vjp_u.h).  Without grad_u this is the launch above, the
// same code object; with it sysid_vjp_u_kernel, whose lanes own the p + m columns of [E | G] and whose pool row is longer.
template <class Mdl>
int sysid_rollout_vjp_u(int B, int T, const double* x, const double* u, const double* th, int tb, const double* gx, double* grad_theta, double* grad_x0, double* grad_u,
                        void* st) {
    if (B <= 0 || T <= 0 || !x || !u || !th || !gx || (!grad_theta && !grad_x0 && !grad_u) || (tb != 0 && tb < Mdl::NP)) return PDP_E_ARG;
    if (!grad_u) return sysid_rollout_vjp<Mdl>(B, T, x, u, th, tb, gx, grad_theta, grad_x0, st);
    const auto pl = sweep_plan<Mdl, SysidVjpUPool, sweep_fits_pm<Mdl>>(B);
    if constexpr (!pl.ok) return pl.rows;
    else return pl.rows < 0 ? pl.rows : launch(sysid_vjp_u_kernel<Mdl>, dim3(B), dim3(64), pl.lds, S(st), B, T, x, u, th, tb, gx, grad_theta, grad_x0, grad_u, pl.rows);
}
// pool rows of the launch above (pdp_sysid_rollout_vjp_u_rows)
template <class Mdl> int sysid_rollout_vjp_u_rows(int B) { return B <= 0 ? PDP_E_ARG : sweep_plan<Mdl, SysidVjpUPool, sweep_fits_pm<Mdl>>(B).rows; }

// The rollout's Jacobian-vector product (pdp_sysid_rollout_jvp_batched, include/pdp_hip_sysid_jvp.h): one launch of sysid_jvp_kernel on the given trajectory, the
// instantiation with `pathu` when d_u is given.  The pool and the plan are sysid_vjp_kernel's; with d_u the limit is p + m <= 512 as for sysid_vjp_u_kernel.
template <class Mdl>
int sysid_rollout_jvp(int B, int T, const double* x, const double* u, const double* th, int tb, const double* dth, int dtb, const double* dx0, const double* du,
                      double* dx, void* st) {
    if (B <= 0 || T <= 0 || !x || !u || !th || !dx || (!dth && !dx0 && !du) || (tb != 0 && tb < Mdl::NP) || (dtb != 0 && dtb < Mdl::NP)) return PDP_E_ARG;
    const auto pl = sweep_plan<Mdl, SysidVjpPool, sweep_fits_p<Mdl>>(B);
    if constexpr (!pl.ok) return pl.rows;
    else return pl.rows < 0 ? pl.rows : with_bool(du != nullptr, [&](auto WU) {
        if constexpr (WU() && !sweep_fits_pm<Mdl>) return (int)PDP_E_SIZE;
        else return launch(sysid_jvp_kernel<Mdl, WU()>, dim3(B), dim3(64), pl.lds, S(st), B, T, x, u, th, tb, dth, dtb, dx0, du, dx, pl.rows);
    });
}
// pool rows of the launch above (pdp_sysid_rollout_jvp_rows)
template <class Mdl> int sysid_rollout_jvp_rows(int B) { return B <= 0 ? PDP_E_ARG : sweep_plan<Mdl, SysidVjpPool, sweep_fits_p<Mdl>>(B).rows; }

template <class Mdl> int nnz_path() { return Mdl::PATH_NVAR; }

// what the Gauss-Newton entry points of SysID.step check first: sizes, the pointers every one of them needs, no flag but PDP_GRAD_SKIP_MISSING
inline bool sysid_gn_args_ok(int B, int T, const double* u, const double* x_obs, const double* theta, const double* loss, const double* packed, int flags) {
    return B > 0 && T > 0 && u && x_obs && theta && loss && packed && !(flags & ~PDP_GRAD_SKIP_MISSING);
}

}  // namespace

extern "C" {

void pdp_model_get_info(pdp_model_info* info) {
    if (!info) return;
    info->kind = PdpModel::KIND; info->n = PdpModel::NX; info->m = PdpModel::NU; info->p = PdpModel::NP;
    info->nnz_path = nnz_path<PdpModel>(); info->chunk = PdpModel::CHUNK; info->name = PdpModel::NAME;
}
int pdp_oc_rollout_batched(int B, int T, const double* x0, const double* u, const double* theta, int tb, double* x, double* cost, void* stream) {
    return oc_rollout<PdpModel>(B, T, x0, u, theta, tb, x, cost, stream);
}
int pdp_oc_rollout_feedback_batched(int B, int T, const double* x0, const double* ubar, const double* xbar, const double* gains, const double* alpha,
                                    const double* theta, int tb, double* x, double* u, double* cost, void* stream) {
    return oc_rollout_fb<PdpModel>(B, T, x0, ubar, xbar, gains, alpha, theta, tb, x, u, cost, stream);
}
int pdp_oc_ms_residuals_batched(int B, int T, const double* x, const double* u, const double* lam, const double* theta, int tb, double* c, double* rx,
                                double* ru, double* cost, void* stream) {
    return oc_ms_residuals<PdpModel>(B, T, x, u, lam, theta, tb, c, rx, ru, cost, stream);
}
int pdp_oc_costate_batched(int B, int T, const double* x, const double* u, const double* theta, int tb, double* lam, void* stream) {
    return oc_costate<PdpModel>(B, T, x, u, theta, tb, lam, stream);
}
int pdp_oc_auxsys_batched(int B, int T, const double* x, const double* u, const double* lam, const double* theta, int tb, const pdp_oc_auxsys* out,
                          void* stream) {
    return oc_auxsys<PdpModel>(B, T, x, u, lam, theta, tb, out, stream);
}
int64_t pdp_oc_solve_workspace_bytes(int B, int T, int ls_trials) {
    if constexpr (PdpModel::KIND == PDP_KIND_OC) return OcSolveWs<PdpModel>(nullptr, B, T, ls_trials > 0 ? ls_trials : 10).bytes; else return 0;
}
int pdp_oc_solve_batched(int B, int T, const double* x0, const double* theta, int tb, double* u, double* x, double* lam, double* cost,
                         double* grad_norm, int32_t* converged, double* gains, const pdp_oc_solve_opts* opts, int* iterations, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    return oc_solve<PdpModel>(B, T, x0, theta, tb, u, x, lam, cost, grad_norm, converged, gains, opts, iterations, workspace, workspace_bytes, stream);
}
int64_t pdp_oc_solve_ms_workspace_bytes(int B, int T, int max_iter) { return oc_solve_ms_ws_bytes<PdpModel>(B, T, max_iter); }
int pdp_oc_solve_ms_batched(int B, int T, const double* x0, const double* theta, int tb, double* x, double* u, double* lam, double* cost,
                            double* resid, int32_t* converged, int32_t* iterations, int32_t* status, double* gains, double* iter_log,
                            const pdp_oc_ms_opts* opts, void* workspace, int64_t workspace_bytes, void* stream) {
    return oc_solve_ms<PdpModel>(B, T, x0, theta, tb, x, u, lam, cost, resid, converged, iterations, status, gains, iter_log, opts, workspace, workspace_bytes,
                                 stream);
}
int64_t pdp_oc_pdp_workspace_bytes(int B, int T) {
    if constexpr (PdpModel::KIND == PDP_KIND_OC) return oc_ws_bytes<PdpModel>(B, T); else return 0;
}
int pdp_oc_pdp_grad_batched(int B, int T, int flags, const double* x0, const double* u, const double* theta, int tb, const double* demo_x,
                            const double* demo_u, double* x, double* lam, double* loss, double* grad, double* dxdp, double* dudp, int32_t* status,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    return oc_pdp<PdpModel>(B, T, flags, x0, u, theta, tb, demo_x, demo_u, x, lam, loss, grad, dxdp, dudp, nullptr, nullptr, status, workspace, workspace_bytes, stream);
}
int64_t pdp_oc_riccati_doubles(void) {
    if constexpr (PdpModel::KIND == PDP_KIND_OC) return oc_riccati_doubles<PdpModel>(); else return 0;
}
int64_t pdp_oc_predict_record_floats(void) {
    if constexpr (PdpModel::KIND == PDP_KIND_OC) return PredRec<PdpModel>::SIZE; else return 0;
}
int pdp_oc_pdp_grad_sens_batched(int B, int T, int flags, const double* x0, const double* u, const double* theta, int tb, const double* demo_x,
                                 const double* demo_u, double* x, double* lam, double* loss, double* grad, const pdp_oc_sens_out* sens,
                                 int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    const pdp_oc_sens_out none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const pdp_oc_sens_out& so = sens ? *sens : none;
    if (so.grad_x0)
        return oc_pdp_x0<PdpModel>(B, T, flags, x0, u, theta, tb, demo_x, demo_u, x, lam, loss, grad, so, status, workspace, workspace_bytes, stream);
    return oc_pdp<PdpModel>(B, T, flags, x0, u, theta, tb, demo_x, demo_u, x, lam, loss, grad, so.dxdp, so.dudp, so.riccati, so.predict_record, status, workspace,
                            workspace_bytes, stream);
}
int pdp_oc_predict_record_batched(int B, int T, const double* dtheta, int dtheta_bstride, const float* predict_record, double* x, double* u, double* lam,
                                  void* stream) {
    return oc_predict_rec<PdpModel>(B, T, dtheta, dtheta_bstride, predict_record, x, u, lam, stream);
}
int pdp_oc_predict_batched(int B, int T, const double* dtheta, int dtheta_bstride, const double* dxdp, const double* dudp, const double* riccati, double* x,
                           double* u, double* lam, void* stream) {
    return oc_predict<PdpModel>(B, T, dtheta, dtheta_bstride, dxdp, dudp, riccati, x, u, lam, stream);
}
int pdp_cp_integrate_batched(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* theta, int tb, double* x, double* u,
                             double* cost, void* stream) {
    if (cp_cot(pol)) return cp_cot_refusal();
    return cp_integrate<PdpModel>(B, T, pol, p, x0, theta, tb, x, u, cost, stream);
}
int pdp_cp_auxsys_batched(int B, int T, const pdp_policy* pol, int p, const double* x, const double* u, const double* theta, int tb, double* dynF,
                          double* dynG, double* dUx, double* dUe, double* dcx, double* dcu, double* dhx, void* stream) {
    if (cp_cot(pol)) return cp_cot_refusal();
    return cp_auxsys<PdpModel>(B, T, pol, p, x, u, theta, tb, dynF, dynG, dUx, dUe, dcx, dcu, dhx, stream);
}
int64_t pdp_cp_step_workspace_bytes(int B, int T, const pdp_policy* pol, int p) { return cp_cot(pol) ? 0 : cp_step_ws_bytes<PdpModel>(B, T, pol, p); }
int pdp_cp_step_batched(int B, int T, const pdp_policy* pol, int p, const double* x0, const double* theta, int tb, double* loss, double* grad,
                        double* x, double* u, void* workspace, int64_t workspace_bytes, void* stream) {
    if (pol && (pol->kind & PDP_POLICY_TANGENT)) return cp_jvp<PdpModel>(B, T, (const pdp_policy_tan*)pol, p, theta, tb, loss, grad, x, u, stream);
    if (cp_cot(pol)) return cp_vjp<PdpModel>(B, T, (const pdp_policy_cot*)pol, p, theta, tb, loss, grad, x, u, stream);
    return cp_step<PdpModel>(B, T, pol, p, x0, theta, tb, loss, grad, x, u, workspace, workspace_bytes, stream);
}
int pdp_sysid_integrate_batched(int B, int T, const double* x0, const double* u, const double* theta, int tb, double* x, void* stream) {
    return sysid_integrate<PdpModel>(B, T, x0, u, theta, tb, x, stream);
}
int pdp_sysid_auxsys_batched(int B, int T, const double* x, const double* u, const double* theta, int tb, double* dynF, double* dynE, void* stream) {
    return sysid_auxsys<PdpModel>(B, T, x, u, theta, tb, dynF, dynE, stream);
}
int pdp_sysid_step_batched(int B, int T, const double* u, const double* x_obs, const double* theta, int tb, double* loss, double* grad, void* stream) {
    return sysid_step<PdpModel>(B, T, u, x_obs, theta, tb, loss, grad, nullptr, 0, stream);
}
int64_t pdp_sysid_step_workspace_bytes(int B, int T) { return sysid_step_ws_bytes<PdpModel>(B, T); }
int pdp_sysid_step_ws_batched(int B, int T, const double* u, const double* x_obs, const double* theta, int tb, double* loss, double* grad, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    return sysid_step<PdpModel>(B, T, u, x_obs, theta, tb, loss, grad, workspace, workspace_bytes, stream);
}
int pdp_sysid_step_gn_batched(int B, int T, const double* u, const double* x_obs, const double* x0, const double* theta, int tb, int flags, double* loss, double* packed,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    if (!sysid_gn_args_ok(B, T, u, x_obs, theta, loss, packed, flags)) return PDP_E_ARG;
    return (flags & PDP_GRAD_SKIP_MISSING) ? sysid_step<PdpModel, PDP_SYSID_GN_MISS>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0)
                                           : sysid_step<PdpModel, PDP_SYSID_GN>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0);
}
int pdp_sysid_step_gn_ini_batched(int B, int T, const double* u, const double* x_obs, const double* x0, int ini_mask, const double* theta, int tb, int flags, double* loss,
                                  double* packed, void* workspace, int64_t workspace_bytes, void* stream) {
    if (ini_mask == 0) return pdp_sysid_step_gn_batched(B, T, u, x_obs, x0, theta, tb, flags, loss, packed, workspace, workspace_bytes, stream);
    if (!sysid_gn_args_ok(B, T, u, x_obs, theta, loss, packed, flags)) return PDP_E_ARG;
    if (PdpModel::NX < 32 && ((unsigned)ini_mask >> PdpModel::NX) != 0) return PDP_E_ARG;       // a mask bit >= n
    const unsigned mask = (unsigned)ini_mask;
    return (flags & PDP_GRAD_SKIP_MISSING)
               ? sysid_step<PdpModel, PDP_SYSID_GN_INI_MISS>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0, mask)
               : sysid_step<PdpModel, PDP_SYSID_GN_INI>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0, mask);
}
int pdp_sysid_step_wls_batched(int B, int T, const double* u, const double* x_obs, const double* x0, int ini_mask, const double* weights, int64_t weights_bstride,
                               double huber_delta, const double* theta, int tb, int flags, double* loss, double* packed, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    if (!sysid_gn_args_ok(B, T, u, x_obs, theta, loss, packed, flags)) return PDP_E_ARG;
    if (!(huber_delta > 0.0)) return PDP_E_ARG;                                                  // (<= 0 and NaN)
    if (weights_bstride != 0 && weights_bstride != (int64_t)(T + 1) * PdpModel::NX) return PDP_E_ARG;
    if (PdpModel::NX < 32 && ((unsigned)ini_mask >> PdpModel::NX) != 0) return PDP_E_ARG;       // a mask bit >= n
    const unsigned mask = (unsigned)ini_mask;
    // without weights the kernels load x_obs in their place (a readable block of the same shape) and select 1.0
    const SysidWls wls{weights ? weights : x_obs, weights ? (long long)weights_bstride : (long long)(T + 1) * PdpModel::NX, huber_delta, weights ? 1 : 0,
                       (flags & PDP_GRAD_SKIP_MISSING) ? 1 : 0};
    return mask ? sysid_step<PdpModel, PDP_SYSID_GN_W_INI>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0, mask, wls)
                : sysid_step<PdpModel, PDP_SYSID_GN_W>(B, T, u, x_obs, theta, tb, loss, packed, workspace, workspace_bytes, stream, x0, 0u, wls);
}
int pdp_sysid_rollout_vjp_batched(int B, int T, const double* x, const double* u, const double* theta, int tb, const double* grad_x, double* grad_theta,
                                  double* grad_x0, void* stream) {
    return sysid_rollout_vjp<PdpModel>(B, T, x, u, theta, tb, grad_x, grad_theta, grad_x0, stream);
}
int pdp_sysid_rollout_vjp_u_batched(int B, int T, const double* x, const double* u, const double* theta, int tb, const double* grad_x, double* grad_theta,
                                    double* grad_x0, double* grad_u, void* stream) {
    return sysid_rollout_vjp_u<PdpModel>(B, T, x, u, theta, tb, grad_x, grad_theta, grad_x0, grad_u, stream);
}
int pdp_sysid_rollout_vjp_u_rows(int B) { return sysid_rollout_vjp_u_rows<PdpModel>(B); }
int pdp_sysid_rollout_jvp_batched(int B, int T, const double* x, const double* u, const double* theta, int tb, const double* d_theta, int d_theta_bstride,
                                  const double* d_x0, const double* d_u, double* d_x, void* stream) {
    return sysid_rollout_jvp<PdpModel>(B, T, x, u, theta, tb, d_theta, d_theta_bstride, d_x0, d_u, d_x, stream);
}
int pdp_sysid_rollout_jvp_rows(int B) { return sysid_rollout_jvp_rows<PdpModel>(B); }
int pdp_oc_pdp_grad_wls_batched(int B, int T, int flags, const double* x0, const double* u, const double* theta, int theta_bstride, const double* demo_x,
                                const double* demo_u, const double* weights_x, int64_t weights_x_bstride, const double* weights_u, int64_t weights_u_bstride,
                                double huber_delta, double* x, double* lam, double* loss, double* packed, int32_t* status, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    return oc_pdp_wls<PdpModel>(B, T, flags, x0, u, theta, theta_bstride, demo_x, demo_u, weights_x, weights_x_bstride, weights_u, weights_u_bstride, huber_delta, x, lam,
                                loss, packed, status, workspace, workspace_bytes, stream);
}

}  // extern "C"
