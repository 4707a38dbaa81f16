"""The reference's gradient-descent loops kept on the device and replayed as ONE hipGraph per iteration: IRLLoop (solve + PDP gradient + update) and GDLoop (any fused
step + update: SysID.step, ControlPlanning.step).

Reference loop (Examples/IRL/cartpole/cartpole_PDP.py:52-80, Examples/IRL/quadrotor/uav_PDP.py:52-62): at the current parameter solve every demonstration's OC problem
(`OCSys.ocSolver`), differentiate the solutions (`getAuxSys` + `lqrSolver`), chain rule against the demonstrations, `theta <- theta - lr * mean gradient`.  Here an
iteration is two kernels - the multiple-shooting solve from the first-order prediction of its solution (pdp_oc_solve_ms_batched with PDP_MS_PREDICT, in place on the previous
solution), the fused gradient unit that also leaves the prediction record for the next solve (pdp_oc_pdp_grad_sens_batched), and the parameter update with its traces
and counters (pdp_gd_update_batched: one launch).  Nothing in the loop waits for the host: loss and parameter traces are written into device arrays (a device-side counter indexes them), convergence
flags and iteration counts of the solves are accumulated on the device and read once at the end.  `IRLLoop.capture()` records the iteration once (torch.cuda.CUDAGraph =
hipGraph on ROCm: every buffer, the parameter vector, the step and the traces live at fixed device addresses) and `IRLLoop.run(n)` replays it n times.  Measured
(bench.py, `irl_loop_wall_clock`): with three launches per iteration and no synchronisation the Python-driven loop keeps the GPU as busy as the graph replay does (C3: 0.236 /
0.245 ms per iteration, C2: 0.096 / 0.100 ms); the graph is for callers whose host thread is busy elsewhere.

LMLoop / lm_step: the same IRL problem as nonlinear least squares.  The loss of the drivers is a sum of squares, and the fused unit's PDP_GRAD_GAUSS_NEWTON instantiation returns
the Gauss-Newton matrix G = J'J beside the gradient J'r from the sensitivity tiles it holds anyway, so a Levenberg-Marquardt step costs one solve and one unit call, like a
gradient-descent step, and a handful of them reach what thousands of descent steps do not.  A step is accepted or rejected on the loss: this loop is driven by the host (LMLoop.for_irl reads
the device once per evaluation: rows and health flags in one copy) and is not graph-replayed.  LMLoop.for_sysid is the same loop on SysID.step, whose loss is a sum of
squares with no inner solve: one launch per evaluation (pdp_sysid_step_gn_batched), complete or partial (NaN) data.

BatchedLMLoop: MANY independent least-squares problems - a parameter estimate per unit of a fleet, per demonstrator, per segment, per bootstrap resample - advanced in
lock-step on the device.  The fused units take per-sample parameters and write one row per trajectory anyway; here an evaluation is one launch of the unit for all problems and
one launch of pdp_lm_update_batched (csrc/pdp_lm_kernels.h) does for all of them what LMLoop.step does on the host.  The host reads an 8-byte counter every few iterations.
"""
import numpy as np

from . import runtime as rt
from .abi import PDP_MS_PREDICT_REJECTED, PDP_MS_RESTORED, PDP_MS_SOC, PDP_MS_WATCHDOG


class _DeviceLoop:
    """what the device-resident loops share: the parameter vector, its step, traces and counters at fixed device addresses, graph capture and replay"""

    def _init_state(self, p, theta0, lr, max_steps):
        torch = rt.torch_cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        self.lr = float(lr)
        self.theta = rt.dev(np.asarray(theta0, dtype=float).reshape(-1)).clone()
        assert self.theta.numel() == p
        self.dtheta = torch.zeros(p, **f64)
        self.max_steps = int(max_steps)
        self.loss_trace = torch.zeros(self.max_steps, **f64)
        self.parameter_trace = torch.zeros(self.max_steps, p, **f64)
        # device-side counters (pdp_gd_update_batched): iterations done (indexes the traces) | OC solves that did not converge | trajectories on which a Riccati sweep
        # reported numerical trouble | Newton iterations of all OC solves
        self.counters = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.graph = None
        self.steps_done = 0

    def _started(self):
        return True

    def start(self):
        pass

    def capture(self, warmup=2):
        """record step() as a graph (after `warmup` eager iterations on a side stream, as torch asks for).  The warm-up iterations are real iterations of the loop
        (they advance theta, the traces and steps_done): run() passes the number it still owes so that a short run is never overshot."""
        torch = rt.torch_cuda()
        if not self._started():
            self.start()
        assert self.steps_done + warmup <= self.max_steps, "traces are full: raise max_steps"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step()
                self.steps_done += 1
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.step()                     # (capturing executes nothing)
        return self

    def run(self, n, graphed=True):
        """n more iterations: graph replays (capture() first) or eager steps.  Returns the number of iterations done so far."""
        if not self._started():
            self.start()
            n -= 1
        assert self.steps_done + n <= self.max_steps, "traces are full: raise max_steps"
        if graphed:
            if self.graph is None and n > 0:
                before = self.steps_done
                self.capture(warmup=min(2, n))
                n -= self.steps_done - before
                assert n >= 0
            for _ in range(max(n, 0)):
                self.graph.replay()
        else:
            for _ in range(max(n, 0)):
                self.step()
        self.steps_done += max(n, 0)
        return self.steps_done

    def results(self):
        """host copies (one synchronisation): the reference's result fields + the health counters"""
        k, unconverged, trouble, newton = (int(v) for v in self.counters.cpu().numpy())
        return {"loss_trace": self.loss_trace[:k].cpu().numpy(), "parameter_trace": self.parameter_trace[:k].cpu().numpy(), "learning_rate": self.lr,
                "iterations": k, "unconverged_solves": unconverged, "riccati_trouble": trouble, "newton_iterations": newton}


class GDLoop(_DeviceLoop):
    """The gradient-descent loop of the reference's SysID and planning drivers (Examples/SysID/*/..._PDP.py, PDP.py:1261-1296: loss, dp = step(...); parameter -= lr * dp
    with the batch means of PDP.py:1293-1294) around ANY fused step: step_fn(theta [p], a CUDA tensor that is updated in place) -> (loss [B], grad [B, p]) CUDA tensors,
    e.g.  lambda th: mdl.sysid_step(u, x_obs, th)  or  lambda th: mdl.cp_step(pol, p, x0, th, T).  Two launches per iteration (the step and pdp_gd_update_batched), no host
    synchronisation, recordable as a hipGraph."""

    def __init__(self, step_fn, theta0, lr, max_steps=100000):
        self.step_fn = step_fn
        self._init_state(int(np.asarray(theta0).size), theta0, lr, max_steps)

    def step(self):
        loss, grad = self.step_fn(self.theta)[:2]
        rt.gd_update(loss, grad, self.lr, self.theta, self.dtheta, self.counters, loss_trace=self.loss_trace, parameter_trace=self.parameter_trace)


class IRLLoop(_DeviceLoop):
    """mdl: runtime.ModelLib of an OC model (PDP.OCSys.model() or zoo.get(system, "irl")); demo_x [B, T+1, n], demo_u [B, T, m]: the demonstrations; theta0 [p]: the initial
    parameter (shared by all demonstrations, as in the reference); lr: learning rate; record: "full" (states, controls and multipliers are predicted) or "primal"
    (states and controls only: cheaper, enough where the multipliers move little per step); max_steps: length of the on-device traces; guard (default): every solve
    checks its predicted start against the previous solution and starts from the better one (PDP_MS_PREDICT_GUARD) - the first iterations of the reference's stored
    rocket run take parameter steps across which the unguarded prediction leads Newton's method to another stationary point (tests/test_gpu_gd_replay.py)."""

    def __init__(self, mdl, demo_x, demo_u, theta0, lr, record="full", tol=1e-10, max_iter=300, max_steps=100000, guard=True):
        assert record in ("full", "primal")
        self.mdl, self.tol, self.max_iter, self.primal, self.guard = mdl, float(tol), int(max_iter), record == "primal", bool(guard)
        self.demo_x, self.demo_u = rt.dev(demo_x), rt.dev(demo_u)
        self.B, self.T = int(self.demo_u.shape[0]), int(self.demo_u.shape[1])
        assert self.demo_x.shape == (self.B, self.T + 1, mdl.n) and self.demo_u.shape == (self.B, self.T, mdl.m)
        self.x0 = self.demo_x[:, 0].contiguous()
        self._init_state(mdl.p, theta0, lr, max_steps)
        self.sol = None                                                            # (x, u, lam) of the current parameter: the solver works in place on them
        self.bufs = {}                                                             # outputs of the gradient unit (fixed addresses)

    def _started(self):
        return self.sol is not None

    # ---- one iteration, no host synchronisation anywhere
    def _update(self, out, sol):
        # mean loss and gradient, theta <- theta - lr * mean gradient, dtheta (also the step the next solve's prediction is made for), traces, counters: ONE launch
        # (as tensor operations this was fourteen small kernels - 70 us per iteration, a quarter of a C3 iteration)
        rt.gd_update(out["loss"], out["grad"], self.lr, self.theta, self.dtheta, self.counters, status=out["status"], converged=sol["converged_flags"],
                     iterations=sol["iterations"], loss_trace=self.loss_trace, parameter_trace=self.parameter_trace)

    def _gradient(self):
        x, u, lam = self.sol
        return self.mdl.oc_pdp_grad(u, self.theta, self.demo_x, self.demo_u, x=x, lam=lam, want_predict_record="primal" if self.primal else True, buffers=self.bufs)

    def start(self):
        """first iteration: cold solve from the reference's all-zero guess (PDP.py:155,166), gradient, update"""
        s = self.mdl.oc_solve_ms(self.x0, self.theta, self.T, tol=self.tol, max_iter=self.max_iter)
        self.sol = (s["state"], s["control"], s["costate"])
        self._update(self._gradient(), s)
        self.steps_done = 1

    def step(self):
        """one warm iteration: solve at the moved parameter from the predicted start (in place), gradient + record, update"""
        s = self.mdl.oc_solve_ms(self.x0, self.theta, self.T, tol=self.tol, max_iter=self.max_iter, warm=self.sol, consume_warm=True,
                                 predict=dict(dtheta=self.dtheta, record=self.bufs["predict_record"], primal=self.primal, guard=self.guard))
        self._update(self._gradient(), s)

    def results(self):
        r = super().results()
        r["newton_iterations_per_solve"] = r["newton_iterations"] / max(1, r["iterations"] * self.B)
        return r


def lm_step(g, G, lam):
    """Marquardt's scaled damping: step = solve(G + lam diag(diag G), g), a diagonal entry of 0 replaced by lam itself; the trial point is theta - step.  g [p] and G [p, p]
    are host arrays (p <= 16 and G is a batch sum: numpy.linalg.solve on the host, lstsq where the damped matrix is still singular)."""
    g, G = np.asarray(g, dtype=float).reshape(-1), np.asarray(G, dtype=float)
    d = np.diag(G).copy()
    A = G + np.diag(np.where(d == 0.0, lam, lam * d))
    try:
        return np.linalg.solve(A, g)
    except np.linalg.LinAlgError:
        return np.linalg.lstsq(A, g, rcond=None)[0]


def arrow_normal_equations(rows, p, q):
    """The normal equations of ONE shared theta [p] and one unknown initial-state part [q] per recording, from the B augmented rows grad [W] | loss | G [W][W]
    (W = p + q) of sysid_step(estimate_ini=): the unknown vector is [theta | x0_0[idx] | ... | x0_{B-1}[idx]], N = p + B q, and with the mean over the recordings as
    the loss the matrix is arrow-shaped - the theta block and the theta-x0_b blocks are sums over the rows / B, the block of x0_b is row b's own block / B, and two
    different recordings share no entry.  Equal to J'J / B of the stacked dense Jacobian.  rows [B, W + 1 + W W]: a torch tensor on any device (CPU included);
    returns ONE flat tensor grad [N] | loss | G [N][N] on the same device (what goes to the host in one copy)."""
    import torch
    B, W = int(rows.shape[0]), p + q
    N = p + B * q
    g, loss, G = rows[:, :W], rows[:, W], rows[:, W + 1:].reshape(B, W, W)
    out = rows.new_zeros(N + 1 + N * N)
    out[:p] = g[:, :p].sum(dim=0) / B
    out[p:N] = (g[:, p:] / B).reshape(-1)
    out[N] = loss.sum() / B
    A = out[N + 1:].view(N, N)
    A[:p, :p] = G[:, :p, :p].sum(dim=0) / B
    A[:p, p:] = (G[:, :p, p:] / B).permute(1, 0, 2).reshape(p, B * q)
    A[p:, :p] = (G[:, p:, :p] / B).reshape(B * q, p)
    b = torch.arange(B, device=rows.device)
    A[p:, p:].unflatten(0, (B, q)).unflatten(2, (B, q))[b, :, b, :] = G[:, p:, p:] / B
    return out


def bad_irl_samples(solve, out):
    """The samples of an IRL evaluation that must not be used, bool [B] on the device (no synchronisation): the solve did not converge, it set a status bit other than
    the informational ones, or the fused unit set a status bit.  solve: the dict of oc_solve_ms, out: the dict of the unit."""
    informational = PDP_MS_RESTORED | PDP_MS_PREDICT_REJECTED | PDP_MS_SOC | PDP_MS_WATCHDOG
    return (solve["converged_flags"] == 0) | ((solve["status"] & ~informational) != 0) | (out["status"] != 0)


def non_finite_rows(rows):
    """bool [B] on the device of `rows` [B, w]: the rows that hold a non-finite entry (a diverged rollout: SysID has no status word)"""
    return (~rows.isfinite()).any(dim=1)


def _host(a):
    return np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, dtype=float)


def prior_layout(who, mean_shape, precision_shape, p, K=None, prior_kind=None):
    """0 (the precision is a diagonal) or 1 (a full matrix) from the shapes of a prior: mean [p] (or [K, p] where K is given); precision [p] or [p, p], with K also
    [K, p] and [K, p, p].  Where K == p the shape [p, p] says nothing - a shared full matrix or one diagonal per problem: prior_kind ("diagonal" or "full") decides,
    and without it the shape is refused rather than guessed.  A shape that is none of these, or one that contradicts prior_kind, is a ValueError."""
    if prior_kind not in (None, "diagonal", "full"):
        raise ValueError("%s: prior_kind is 'diagonal' or 'full'" % who)
    ps = tuple(int(v) for v in precision_shape)
    if K is not None and K == p and ps == (p, p) and prior_kind is None:
        raise ValueError("%s: with K == p = %d a prior_precision of shape [%d, %d] is a shared full matrix or one diagonal per problem: say prior_kind='full' or "
                         "prior_kind='diagonal'" % (who, p, p, p))
    try:
        kind = rt.lm_prior_shapes(mean_shape, ps, K if K is not None else -1, p, diagonal_per_problem=prior_kind == "diagonal")[0]
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e)) from None
    if prior_kind is not None and kind != (0 if prior_kind == "diagonal" else 1):
        raise ValueError("%s: prior_precision of shape %s is not a %s precision" % (who, list(ps), prior_kind))
    return kind


def check_prior(who, prior_mean, prior_precision, p, K=None, prior_kind=None):
    """The prior_mean / prior_precision keywords of the least-squares loops, checked on the host before any launch: (mean, precision) as fp64 numpy arrays, or (None,
    None) when neither is given.  Shapes and prior_kind: prior_layout; a non-finite entry, a negative diagonal entry or an asymmetric matrix is a ValueError."""
    if prior_mean is None and prior_precision is None:
        return None, None
    if prior_mean is None or prior_precision is None:
        raise ValueError("%s: prior_mean and prior_precision go together" % who)
    mean, prec = _host(prior_mean), _host(prior_precision)
    kind = prior_layout(who, mean.shape, prec.shape, p, K, prior_kind)
    if not (np.isfinite(mean).all() and np.isfinite(prec).all()):
        raise ValueError("%s: prior_mean / prior_precision hold a non-finite entry" % who)
    if kind == 1 and not np.array_equal(prec, np.swapaxes(prec, -1, -2)):
        raise ValueError("%s: prior_precision is not symmetric" % who)
    if ((np.diagonal(prec, axis1=-2, axis2=-1) if kind == 1 else prec) < 0).any():
        raise ValueError("%s: prior_precision has a negative diagonal entry" % who)
    return mean, prec


def _prior_with_ini(who, mean, prec, prior_ini_precision, p, q, start, K=None, prior_kind=None):
    """the prior of [theta | estimated initial-state components]: the theta part (checked by check_prior; None: no prior on theta) extended by a diagonal prior
    prior_ini_precision [q] on the components, centred on their starting values `start` - [K, q] with K given (one vector [p + q] per problem), else [B, q] (one vector
    [p + B q]).  Returns (mean, precision, prior_kind of the result) in check_prior's shapes, or (None, None, None)."""
    if prior_ini_precision is None:
        return mean, prec, prior_kind
    pi = _host(prior_ini_precision).reshape(-1)
    if pi.size != q or not np.isfinite(pi).all() or (pi < 0).any():
        raise ValueError("%s: prior_ini_precision is [q] = [%d], finite and >= 0" % (who, q))
    start = np.asarray(start, dtype=float)
    n = start.shape[0]
    if mean is None:
        mean, prec = np.zeros(p), np.zeros(p)
    kind = prior_layout(who, mean.shape, prec.shape, p, K, prior_kind)
    if K is not None:                               # one vector per problem: [K, p + q], the layout named explicitly (K may equal p + q)
        mean_w = np.concatenate([np.broadcast_to(mean, (K, p)), start], axis=1)
        if kind == 0:
            return mean_w, np.concatenate([np.broadcast_to(prec, (K, p)), np.broadcast_to(pi, (K, q))], axis=1), "diagonal"
        full = np.zeros((K, p + q, p + q))
        full[:, :p, :p] = prec
        full[:, np.arange(p, p + q), np.arange(p, p + q)] = pi
        return mean_w, full, "full"
    mean_w = np.concatenate([mean, start.reshape(-1)])
    if kind == 0:
        return mean_w, np.concatenate([prec, np.tile(pi, n)]), "diagonal"
    full = np.zeros((p + n * q, p + n * q))
    full[:p, :p] = prec
    i = np.arange(p, p + n * q)
    full[i, i] = np.tile(pi, n)
    return mean_w, full, "full"


def _sample_count(who, B, n_total, has_prior):
    """the number of samples the loss of a for_* host loop is a mean over: n_total, else B on one rank; under a process group of more than one rank without n_total it
    is only known after the exchange - None, and with a prior (whose precision has to be divided by it before the first evaluation) a ValueError"""
    import torch
    dist = torch.distributed
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if n_total is not None:
        return float(n_total), multi
    if multi and has_prior:
        raise ValueError("%s: a prior under a process group needs n_total (the precision is divided by the total sample count; no collective is issued for it)" % who)
    return (None if multi else float(B)), multi


def _first_row(ini_state, mask_or_idx, n):
    """count_observed's first_row for the states of a rollout: all of row 0 where ini_state was given, the estimated components where some are, else none"""
    if ini_state is not None:
        return True
    if mask_or_idx:
        keep = np.zeros(n, dtype=bool)
        keep[list(mask_or_idx)] = True
        return keep
    return False


def inverse_pivoted(A):
    """(A^-1, ok, pivot_ratio) by the elimination of the device (pdp_lm_covariance_batched): [A | I] reduced with partial pivoting - the largest magnitude of the
    remaining rows, ties to the lowest row, a NaN counting as the largest -, back-substituted per column; ok is False where a pivot is not > 1e-300 in magnitude;
    pivot_ratio is the smallest over the largest pivot magnitude"""
    A = np.array(A, dtype=float)
    n = A.shape[0]
    B, ok, small, large = np.eye(n), True, np.inf, 0.0
    with np.errstate(all="ignore"):
        for c in range(n):
            mag = np.abs(A[c:, c])
            j = c + int(np.argmax(np.where(np.isnan(mag), np.inf, mag)))
            if j != c:
                A[[c, j]], B[[c, j]] = A[[j, c]], B[[j, c]]
            piv = A[c, c]
            ok = ok and bool(abs(piv) > 1e-300)
            small, large = (abs(piv) if abs(piv) < small else small), (abs(piv) if abs(piv) > large else large)
            f = A[c + 1:, c] / piv
            A[c + 1:, c + 1:] = A[c + 1:, c + 1:] - f[:, None] * A[c, c + 1:]
            B[c + 1:] = B[c + 1:] - f[:, None] * B[c]
        for c in range(n - 1, -1, -1):
            B[c] = B[c] / A[c, c]
            B[:c] = B[:c] - A[:c, c][:, None] * B[c]
        return B, ok, float(small / large)


def _covariance_host(G, loss, scale_count, noise, n_observed, p, has_prior, who):
    """Cov of one estimate from its mean-row G (the loss is a sum over scale_count samples divided by it), by the device's rules: cov = scale G^-1 with scale =
    sigma^2 / scale_count from inverse_pivoted; status 1, NaN and pivot_ratio 0 where a pivot fails or an entry of G or of the result is not finite.
    dict(cov, std_err, pivot_ratio, status, sigma2) as numpy"""
    if noise not in ("known", "estimated"):
        raise ValueError("%s.covariance: noise is 'known' or 'estimated'" % who)
    sigma2 = 1.0
    if noise == "estimated":
        if has_prior:
            raise ValueError("%s.covariance: noise='estimated' with a prior - the loss of the row contains the prior's share; give the weights as 1 / sigma^2 and "
                             "use noise='known'" % who)
        N = float(n_observed)
        sigma2 = scale_count * loss / (N - p) if N > p else np.nan
    G = np.asarray(G, dtype=float)
    inv, ok, ratio = inverse_pivoted(G)
    with np.errstate(all="ignore"):
        cov = (sigma2 / scale_count) * inv
        status = 0 if (ok and np.isfinite(G).all() and np.isfinite(cov).all()) else 1
        if status:
            ratio, cov = 0.0, np.full_like(G, np.nan)
        cov = 0.5 * (cov + cov.T)
        d = np.diag(cov)
        std = np.where(d < 0, np.nan, np.sqrt(np.abs(d)))
    return dict(cov=cov, std_err=std, pivot_ratio=ratio, status=status, sigma2=sigma2)


class LMLoop:
    """Levenberg-Marquardt on a sum-of-squares loss.  evaluate(theta [p], numpy) -> (loss, g [p], G [p, p]) as host floats / numpy arrays with g = J'r, G = J'J in the same
    scaling (half the gradient of loss = |r|^2, as the fused unit returns them), or None where theta cannot be evaluated (a solve that did not converge, a singular stage).
    Schedule: the trial point theta - lm_step(g, G, lam) is accepted iff its loss is finite and strictly below the current one; then lam <- max(lam / down, lam_min), else
    lam <- lam * up.  run() ends at max_evals evaluations, at loss <= loss_tol, or when lam > lam_max - no damping the schedule may try improves the loss any more: the fp64
    floor of the problem, reported as results()["stalled"], not raised.
    prior_mean [p], prior_precision [p] (the diagonal) or [p, p]: a Gaussian prior - (theta - mean)' P (theta - mean) is added to the loss, P (theta - mean) to g and P
    to G after every evaluation (hence after an all-reduce inside evaluate, identically on every rank); P is taken as given, in the scale of evaluate's loss (the for_*
    constructors, whose loss is a mean over the samples, divide the natural-unit precision by the sample count).  results()["prior_loss"] is the prior's share of the
    loss at the accepted point.  covariance(): the error bar of the estimate.
    One shared-parameter problem, driven by the host; many independent problems with their own parameters, decided on the device: BatchedLMLoop (below)."""

    def __init__(self, evaluate, theta0, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, prior_mean=None, prior_precision=None):
        self.evaluate = evaluate
        self.theta = np.array(_host(theta0), dtype=float).reshape(-1)
        self.prior_mean, self.prior_precision = check_prior("LMLoop", prior_mean, prior_precision, self.theta.size)
        self.prior_loss = None                  # the prior's share of the loss at self.theta
        self.sample_count = 1.0                 # the loss of evaluate is the natural-unit objective divided by this (the for_* constructors set it)
        self.n_observed = None                  # entries that enter the loss (the for_* constructors set it where it is known without a collective)
        self.lam, self.up, self.down, self.lam_min, self.lam_max = float(lam0), float(up), float(down), float(lam_min), float(lam_max)
        self.current = None                     # (loss, g, G) at self.theta
        self.evaluations = self.rejected = 0
        self.stalled = False
        self.on_accept = None                   # called after every accepted point (for_irl: keeps that point's solution as the next warm start)
        self.loss_trace, self.parameter_trace, self.lambda_trace = [], [], []

    def _eval(self, theta):
        """((loss, g, G) with the prior added, the prior's share of the loss or None), or None where theta cannot be evaluated"""
        self.evaluations += 1
        r = self.evaluate(theta)
        if r is None:
            return None
        loss, g, G, q = float(r[0]), np.asarray(r[1], dtype=float).reshape(-1), np.asarray(r[2], dtype=float), None
        if not np.isfinite(loss):
            return None
        if self.prior_mean is not None:
            d = np.asarray(theta, dtype=float).reshape(-1) - self.prior_mean
            P = self.prior_precision
            Pd = P * d if P.ndim == 1 else P @ d
            q = float(d @ Pd)
            loss, g, G = loss + q, g + Pd, G + (np.diag(P) if P.ndim == 1 else P)
            if not np.isfinite(loss):
                return None
        return (loss, g, G), q

    def start(self):
        """the evaluation at theta0 (the first accepted point)"""
        r = self._eval(self.theta)
        if r is None:
            raise RuntimeError("LMLoop: the initial parameter could not be evaluated")
        self.current, self.prior_loss = r
        self._record()

    def _record(self):
        self.loss_trace.append(self.current[0])
        self.parameter_trace.append(self.theta.copy())
        self.lambda_trace.append(self.lam)
        if self.on_accept is not None:
            self.on_accept()

    def step(self):
        """one trial: True if it was accepted"""
        loss, g, G = self.current
        trial = self.theta - lm_step(g, G, self.lam)
        if np.isfinite(trial).all():
            r = self._eval(trial)
        else:
            r, self.evaluations = None, self.evaluations + 1        # (a trial that cannot be formed still counts against the budget)
        if r is not None and r[0][0] < loss:
            self.theta, (self.current, self.prior_loss) = trial, r
            self.lam = max(self.lam / self.down, self.lam_min)
            self._record()
            return True
        self.rejected += 1
        self.lam *= self.up
        return False

    def run(self, max_evals=50, loss_tol=0.0):
        if self.current is None:
            self.start()
        while self.evaluations < max_evals and self.current[0] > loss_tol:
            if self.lam > self.lam_max:
                self.stalled = True
                break
            self.step()
        return self.results()

    def results(self):
        """the reference's result fields over the ACCEPTED points (loss_trace, parameter_trace) + evaluations, rejected, lambda_trace (the damping after each accepted point),
        stalled"""
        r = {"loss_trace": np.array(self.loss_trace), "parameter_trace": np.array(self.parameter_trace).reshape(len(self.parameter_trace), self.theta.size),
             "lambda_trace": np.array(self.lambda_trace), "evaluations": self.evaluations, "rejected": self.rejected, "stalled": self.stalled,
             "iterations": len(self.loss_trace)}
        if self.prior_mean is not None:
            r["prior_loss"] = self.prior_loss
        return r

    def covariance(self, noise="known", n_observed=None):
        """The covariance of the estimate at the accepted point, from G = J'J there (with a prior: J'J + P, the posterior precision): dict(cov [p, p] symmetrised, std_err
        [p], pivot_ratio, status, sigma2) by the rules of the device (inverse_pivoted: the same elimination, pivot rule and threshold; status 1 with NaN and pivot_ratio 0).  noise="known": the weights are 1 / sigma^2,
        Cov = (count G)^-1 with count the sample count the loss is a mean over (1 for a plain LMLoop(evaluate)).  noise="estimated": sigma^2 = count loss / (N - p) scales
        it, N = n_observed (the for_* constructors know it on one rank; under a process group it has to be given: NotImplementedError otherwise - no collective is
        issued here); N <= p gives NaN; with a prior it is a ValueError (the loss contains the prior's share).  Under Huber weights this is the covariance of the final
        reweighted least-squares problem, not the sandwich estimator."""
        if self.current is None:
            raise RuntimeError("LMLoop.covariance: nothing evaluated yet (run() or start() first)")
        if self.sample_count is None:
            raise NotImplementedError("LMLoop.covariance: the total sample count is only known to the exchange (a process group without n_total): give n_total")
        N = n_observed if n_observed is not None else self.n_observed
        if noise == "estimated" and self.prior_mean is None and N is None:
            raise NotImplementedError("LMLoop.covariance(noise='estimated'): the number of observed entries is not known here (a plain evaluate, or samples spread over "
                                      "a process group): give n_observed")
        return _covariance_host(self.current[2], self.current[0], self.sample_count, noise, N, self.theta.size, self.prior_mean is not None, "LMLoop")

    @classmethod
    def for_irl(cls, mdl, demo_x, demo_u, theta0, tol=1e-10, max_iter=300, n_total=None, ini_state=None, skip_missing=False, weights_state=None, weights_control=None,
                huber_delta=None, prior_mean=None, prior_precision=None, **kw):
        """The IRL drivers' problem: mdl a runtime.ModelLib of an OC model, demo_x [B, T+1, n], demo_u [B, T, m] the demonstrations (this rank's shard under
        torch.distributed; n_total as in parallel.allreduce_mean_packed), theta0 [p] shared by all of them.  evaluate(theta) solves every demonstration's OC problem
        (oc_solve_ms: the first cold, later ones warm from COPIES of the last accepted solution, so that a rejected trial cannot damage it), runs the fused unit once with
        gauss_newton=True on the solutions and hands the packed rows, with the count of samples whose solve did not converge or reported trouble or whose unit set a
        status bit, to parallel.mean_row_checked: one all-reduce when a process group exchanges, one copy of p + 3 + p p doubles to the host.  A trial with such a sample on
        ANY rank is None on EVERY rank (the decision travels with the rows: no rank skips a collective the others issue).
        skip_missing: demonstrations with gaps - a NaN in demo_x / demo_u is an entry that was not observed (PDP_GRAD_SKIP_MISSING: a keyframe every k steps, positions
        without velocities, no recorded controls = demo_u all NaN); loss, gradient and G are formed over the observed entries only.  ini_state [B, n] replaces
        demo_x[:, 0] as the initial state of the solves - needed where the first row of a demonstration is not (fully) observed: with skip_missing a NaN in the initial
        state the solves would start from is a ValueError here, before any launch.
        weights_state ([n], [T+1, n] or [B, T+1, n]), weights_control ([m], [T, m] or [B, T, m]), both >= 0 with 0 = not observed, huber_delta (> 0): the row the loop
        minimises carries the weighted / Huber loss, its exact half derivative and the Gauss-Newton matrix of iteratively reweighted least squares
        (pdp_oc_pdp_grad_wls_batched); the loop itself is unchanged.  They are checked once, here, and the weights stay on the device.
        prior_mean, prior_precision: LMLoop's prior in NATURAL units - the objective is the sum over all demonstrations of their losses + (theta - mean)' P (theta -
        mean); the loop minimises it divided by the total number of demonstrations (n_total, else B; under a process group n_total is then required).  The loop knows the
        number of observed entries (covariance(noise="estimated")) on one rank: every entry of demo_u and of rows 1 .. T of demo_x with a weight > 0 that is not a NaN
        under skip_missing, and row 0 of demo_x where ini_state was given (else its residual is identically zero)."""
        prior_mean, prior_precision = check_prior("LMLoop.for_irl", prior_mean, prior_precision, mdl.p)
        count, multi = _sample_count("LMLoop.for_irl", int(np.shape(demo_u)[0]), n_total, prior_mean is not None)
        if skip_missing:                            # judged on what the caller gave (a host array is not moved to the device first)
            rt.refuse_nan_initial_state("LMLoop.for_irl", demo_x, ini_state, "demo_x")
        rows, held = mdl.oc_rows_prepared(demo_x, demo_u, skip_missing, weights_state, weights_control, huber_delta)
        from . import parallel
        demo_x, demo_u = held["demo_x"], held["demo_u"]
        B, T, p = int(demo_u.shape[0]), int(demo_u.shape[1]), mdl.p
        assert demo_x.shape == (B, T + 1, mdl.n) and demo_u.shape == (B, T, mdl.m)
        x0 = (demo_x[:, 0] if ini_state is None else rt.dev(ini_state).reshape(B, mdl.n)).contiguous()
        state = {"accepted": None, "trial": None}

        def evaluate(theta):
            # no decision on this rank's own flags: solve and unit always run, the flags are counted on the device and travel with the rows, so that every rank issues
            # the same collective and takes the same decision (parallel.mean_row_checked) - and the host reads the device once
            s = mdl.oc_solve_ms(x0, theta, T, tol=tol, max_iter=max_iter, warm=state["accepted"])
            out = rows(s["control"], theta, x=s["state"], lam=s["costate"])
            row = parallel.mean_row_checked(out["packed_gn"], bad_irl_samples(s, out), n_total)
            if row is None:
                return None
            state["trial"] = (s["state"], s["control"], s["costate"])
            return float(row[p]), row[:p].copy(), row[p + 1:].reshape(p, p).copy()

        loop = cls(evaluate, theta0, prior_mean=prior_mean, prior_precision=None if prior_precision is None else prior_precision / count, **kw)
        loop.on_accept = lambda: state.update(accepted=state["trial"])
        loop.sample_count = count
        if not multi:
            loop.n_observed = int((rt.count_observed(demo_x, weights_state, skip_missing, _first_row(ini_state, None, mdl.n)) +
                                   rt.count_observed(demo_u, weights_control, skip_missing)).sum().item())
        return loop

    @classmethod
    def for_sysid(cls, mdl, inputs, states, theta0, n_total=None, ini_state=None, skip_missing=False, estimate_ini=None, weights=None, huber_delta=None,
                  prior_mean=None, prior_precision=None, prior_ini_precision=None, **kw):
        """The SysID drivers' problem (Examples/SysID/*/..._PDP.py) as nonlinear least squares: mdl a runtime.ModelLib of a SysID model, inputs [B, T, m] and states
        [B, T+1, n] the recorded data (this rank's shard under torch.distributed; n_total as in parallel.allreduce_mean_packed), theta0 [p] shared by all trajectories.
        evaluate(theta) is ONE launch - sysid_step with gauss_newton=True: loss, gradient and G = J'J from the sensitivity tiles of the fused kernel - and hands the packed
        rows, with the count of rows that hold a non-finite entry (a diverged rollout: SysID has no status word), to parallel.mean_row_checked: one all-reduce when a
        process group exchanges, one copy of p + 3 + p p doubles to the host; a trial with such a row on ANY rank is None on EVERY rank.
        skip_missing: partial data - a NaN in `states` is an entry that was not observed (encoders without velocities, a sample every k steps); ini_state [B, n] replaces
        states[:, 0] as the initial state of the rollouts, needed where the first row is not fully observed (a NaN there is a ValueError before any launch).
        estimate_ini (state indices or a bool mask [n], runtime.ini_indices): these q components of every recording's initial state are unknowns too - one shared theta
        and one unknown initial-state part per recording.  The unknown vector is [theta | x0_0[idx] | ... | x0_{B-1}[idx]], N = p + B q; theta0 is [p] (the estimated
        components start from ini_state, or states[:, 0]) or [N].  An evaluation is one launch of sysid_step(estimate_ini=) at (theta, x0); the arrow-shaped normal
        equations are assembled from the B augmented rows on the device (arrow_normal_equations) and go to the host in one copy; a non-finite row makes the point None;
        the solve is lm_step's, dense on the host.  loop.split(vector) -> (theta [p], ini_state [B, n]).  N > 256, n_total, or a process group of more than one rank is a
        ValueError: many recordings, or recordings spread over ranks, are BatchedLMLoop.for_sysid(estimate_ini=)'s problems, one theta per trajectory.
        weights ([n], [T+1, n] or [B, T+1, n], >= 0, 0 = not observed), huber_delta (> 0): the row the loop minimises carries the weighted / Huber loss, its exact half
        derivative and the Gauss-Newton matrix of iteratively reweighted least squares (ModelLib.sysid_step, pdp_sysid_step_wls_batched); the loop itself is unchanged.
        They are checked once, here.
        prior_mean, prior_precision ([p]; [p] or [p, p]): LMLoop's prior on theta in NATURAL units - the objective is the sum over all trajectories of their losses +
        (theta - mean)' P (theta - mean); the loop minimises it divided by the total number of trajectories (n_total, else B; under a process group n_total is then
        required).  prior_ini_precision [q] (with estimate_ini): a diagonal prior on the estimated components of every recording's initial state, centred on their
        starting values - it fills the diagonal of the x0_b blocks of the arrow system.  The loop knows the number of observed entries (covariance(noise="estimated")) on
        one rank: rows 1 .. T of `states` with a weight > 0 that are not a NaN under skip_missing, and of row 0 everything where ini_state was given, else the estimated
        components (the residual of the others is identically zero)."""
        idx, _ = rt.ini_indices(estimate_ini, mdl.n)
        prior_mean, prior_precision = check_prior("LMLoop.for_sysid", prior_mean, prior_precision, mdl.p)
        if prior_ini_precision is not None and not idx:
            raise ValueError("LMLoop.for_sysid: prior_ini_precision needs estimate_ini")
        count, multi = _sample_count("LMLoop.for_sysid", int(np.shape(inputs)[0]), n_total, prior_mean is not None)
        rows, held = mdl.sysid_rows_prepared(inputs, states, skip_missing, ini_state, idx, weights, huber_delta, own_x0=bool(idx), who="LMLoop.for_sysid",
                                             data_name="states")
        if idx:                                     # (nothing selected is estimate_ini=None)
            return cls._for_sysid_ini(mdl, rows, held, theta0, n_total, ini_state, skip_missing, idx, weights=weights,
                                      prior=(prior_mean, prior_precision, prior_ini_precision), **kw)
        from . import parallel
        inputs, states = held["u"], held["xobs"]
        B, T, p = int(inputs.shape[0]), int(inputs.shape[1]), mdl.p
        assert states.shape == (B, T + 1, mdl.n) and inputs.shape == (B, T, mdl.m)

        def evaluate(theta):
            out = rows(theta)
            row = parallel.mean_row_checked(out["packed_gn"], non_finite_rows(out["packed_gn"]), n_total)      # (a bad row makes the point None before its sums are read)
            if row is None:
                return None
            return float(row[p]), row[:p].copy(), row[p + 1:].reshape(p, p).copy()

        loop = cls(evaluate, theta0, prior_mean=prior_mean, prior_precision=None if prior_precision is None else prior_precision / count, **kw)
        loop.sample_count = count
        if not multi:
            loop.n_observed = int(rt.count_observed(states, weights, skip_missing, _first_row(ini_state, None, mdl.n)).sum().item())
        return loop

    @classmethod
    def _for_sysid_ini(cls, mdl, rows, held, theta0, n_total, ini_state, skip_missing, idx, weights=None, prior=(None, None, None), **kw):
        """rows, held: the prepared evaluation (checked: an estimated component still needs a finite starting value) with initial states of its own"""
        torch = rt.torch_cuda()
        inputs, states, x0, cols = held["u"], held["xobs"], held["x0"], held["columns"]      # x0 persistent: the estimated components are written into it
        B, T, p, q = int(inputs.shape[0]), int(inputs.shape[1]), mdl.p, len(idx)
        assert states.shape == (B, T + 1, mdl.n) and inputs.shape == (B, T, mdl.m)
        N = p + B * q
        dist = torch.distributed
        if n_total is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise ValueError("LMLoop.for_sysid(estimate_ini=): one shared theta with per-recording initial states lives on one rank (no n_total, no process group of "
                             "more than one rank); independent problems shard over ranks with BatchedLMLoop.for_sysid(estimate_ini=)")
        if N > 256:
            raise ValueError("LMLoop.for_sysid(estimate_ini=): N = p + B q = %d unknowns > 256 (a dense solve on the host); one problem per trajectory is "
                             "BatchedLMLoop.for_sysid(estimate_ini=)" % N)
        ini0 = x0.cpu().numpy().copy()
        th0 = np.asarray(theta0.cpu() if hasattr(theta0, "cpu") else theta0, dtype=float).reshape(-1)
        if th0.size == p:
            th0 = np.concatenate([th0, ini0[:, idx].reshape(-1)])
        if th0.size != N:
            raise ValueError("LMLoop.for_sysid(estimate_ini=): theta0 is [p] = [%d] or [p + B q] = [%d], got %d" % (p, N, th0.size))

        def evaluate(vector):
            v = rt.dev(np.ascontiguousarray(vector, dtype=float))                         # one copy to the device: theta and the estimated components
            x0.index_copy_(1, cols, v[p:].view(B, q))
            out = rows(v[:p])
            flat = arrow_normal_equations(out["packed_gn"], p, q).cpu().numpy()            # one copy to the host
            if not np.isfinite(flat).all():         # every entry of every row is in there, summed or as it is: a non-finite row shows
                return None
            return float(flat[N]), flat[:N].copy(), flat[N + 1:].reshape(N, N).copy()

        def split(vector):
            v = np.asarray(vector, dtype=float).reshape(-1)
            ini = ini0.copy()
            ini[:, idx] = v[p:].reshape(B, q)
            return v[:p].copy(), ini

        mean, prec, _ = _prior_with_ini("LMLoop.for_sysid", prior[0], prior[1], prior[2] if (prior[2] is not None or prior[0] is None) else np.zeros(q), p, q, ini0[:, idx])
        loop = cls(evaluate, th0, prior_mean=mean, prior_precision=None if prec is None else prec / float(B), **kw)
        loop.split = split
        loop.sample_count = float(B)
        loop.n_observed = int(rt.count_observed(states, weights, skip_missing, _first_row(ini_state, idx, mdl.n)).sum().item())
        return loop


class BatchedLMLoop:
    """K independent Levenberg-Marquardt problems in lock-step, every decision on the device.  evaluate_rows(trial [K S, p], a CUDA tensor at a fixed address: the
    per-sample parameters) -> (rows [K S, p + 1 + p p] = grad | loss | G per sample, bad int32 [K S] or None), device tensors, no synchronisation; problem k owns the
    samples k S .. k S + S - 1 (S = samples_per_problem) and its loss, gradient and G are their means.  theta0 [K, p], or [p] with K given: every problem starts there.
    The schedule is LMLoop's, per problem (runtime.lm_update / include/pdp_hip_lm.h: the exact order, and the two differences - a damped matrix that is exactly singular is
    a rejected trial, not a least-squares solve; pivoted elimination).  A problem whose initial point cannot be evaluated is FAILED (LMLoop raises there) and the others go
    on.  step() is one evaluation and one update launch; run() reads counters[1] - problems still START or ACTIVE, one 8-byte copy - every poll_every launches.
    prior_mean ([p] or [K, p]), prior_precision ([p] or [K, p]: the diagonal; [p, p] or [K, p, p]: full; [p, p] where K == p), in NATURAL units: the objective of a problem
    is the sum over its S samples of their losses + (theta - mean)' P (theta - mean).  Where K == p the shape [p, p] does not say which of the two it is: prior_kind
    ("diagonal" or "full") is then required (a ValueError otherwise).  The loop minimises that divided by S - the mean row, as without a prior - and hands
    P / S to the update kernel, which adds the prior inside the same launch (pdp_lm_update_prior_batched); losses, traces and loss_tol are those of the augmented mean
    row, results()["prior_loss"] the prior's share of it.  A non-finite entry, a negative diagonal entry or an asymmetric matrix is a ValueError before any launch.
    Without a prior step() launches pdp_lm_update_batched as before.  covariance(): K error bars for K estimates, one more launch.
    Made for many problems with few samples each; one problem with thousands of samples is LMLoop's job.  Not graph-captured; samples of one problem do not span ranks
    (independent problems shard over ranks without any collective)."""

    def __init__(self, evaluate_rows, theta0, samples_per_problem=1, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, max_evals=50, loss_tol=0.0, trace_len=None,
                 K=None, prior_mean=None, prior_precision=None, prior_kind=None):
        shape = tuple(int(v) for v in np.shape(theta0))
        K_ = shape[0] if len(shape) == 2 else (int(K) if K is not None else 1)
        mean, prec = check_prior("BatchedLMLoop", prior_mean, prior_precision, shape[-1], K_, prior_kind)
        diagonal_per_problem = mean is not None and prec.ndim == 2 and prior_layout("BatchedLMLoop", mean.shape, prec.shape, shape[-1], K_, prior_kind) == 0
        torch = rt.torch_cuda()
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        th = rt.dev(theta0)
        if th.dim() == 1:
            th = th[None].expand(int(K) if K is not None else 1, -1)
        self.theta = th.contiguous().clone()
        self.K, self.p = (int(v) for v in self.theta.shape)
        assert K is None or int(K) == self.K
        self.S = S = int(samples_per_problem)
        assert S >= 1 and 1 <= self.p <= 16, "p <= 16 (one 16-lane row per problem)"
        self.evaluate_rows = evaluate_rows
        self.schedule = dict(up=float(up), down=float(down), lam_min=float(lam_min), lam_max=float(lam_max), loss_tol=float(loss_tol), max_evals=int(max_evals))
        L = int(max_evals) + 1 if trace_len is None else int(trace_len)
        K, p, w = self.K, self.p, self.p + 1 + self.p * self.p
        self.trial = self.theta.repeat_interleave(S, dim=0).contiguous()
        self.lam = torch.full((K,), float(lam0), **f64)
        self.current = torch.zeros((K, w), **f64)
        self.state, self.evaluations, self.rejected, self.accepted = (torch.zeros((K,), **i32) for _ in range(4))
        self.accepted_now = torch.zeros((K * S,), **i32)
        self.loss_trace, self.lambda_trace, self.parameter_trace = torch.zeros((K, L), **f64), torch.zeros((K, L), **f64), torch.zeros((K, L, p), **f64)
        self.counters = torch.tensor([0, K], dtype=torch.int64, device="cuda")
        self.after_update = None                # called after every update launch (for_irl: keeps the accepted solutions as the next warm start, on the device)
        self.launches = 0
        self.prior_mean = self.prior_precision = self.prior_loss = None
        self.prior_diagonal_per_problem = diagonal_per_problem      # (the layout is fixed here, not read from the shape again: K may equal p)
        if mean is not None:
            self.prior_mean, self.prior_precision = rt.dev(mean), rt.dev(prec / float(S))      # (the kernel's scale: that of the mean row)
            self.prior_loss = torch.full((K,), float("nan"), **f64)
        self.n_observed = None                  # int64 [K] on the device: entries that enter the loss of each problem (the for_* constructors set it)

    def step(self):
        """one evaluation of all trial points and one update launch; nothing is read back"""
        rows, bad = self.evaluate_rows(self.trial)
        if self.prior_mean is None:
            rt.lm_update(rows, self.theta, self.trial, self.lam, self.current, self.state, self.evaluations, self.rejected, self.accepted, self.counters, bad=bad,
                         accepted_now=self.accepted_now, loss_trace=self.loss_trace, lambda_trace=self.lambda_trace, parameter_trace=self.parameter_trace, **self.schedule)
        else:
            rt.lm_update_prior(rows, self.theta, self.trial, self.lam, self.current, self.state, self.evaluations, self.rejected, self.accepted, self.counters, bad=bad,
                               accepted_now=self.accepted_now, loss_trace=self.loss_trace, lambda_trace=self.lambda_trace, parameter_trace=self.parameter_trace,
                               prior_mean=self.prior_mean, prior_precision=self.prior_precision, prior_loss=self.prior_loss,
                               diagonal_per_problem=self.prior_diagonal_per_problem, **self.schedule)
        if self.after_update is not None:
            self.after_update()
        self.launches += 1

    def active(self):
        """problems still START or ACTIVE: one 8-byte copy (a synchronisation)"""
        return int(self.counters[1].item())

    def run(self, max_launches=None, poll_every=4):
        """steps until no problem is START or ACTIVE (looked at every poll_every launches), at most max_launches of them and never beyond launch max_evals + 1, after
        which every problem has ended by its budget.  Returns results()."""
        limit = self.schedule["max_evals"] + 1
        todo = limit - self.launches if max_launches is None else min(int(max_launches), limit - self.launches)
        for i in range(max(todo, 0)):
            self.step()
            if (i + 1) % max(1, int(poll_every)) == 0 and self.active() == 0:
                break
        return self.results()

    def results(self):
        """host copies (one synchronisation), per problem: loss_trace, parameter_trace, lambda_trace (lists of K arrays over the ACCEPTED points, cut at the trace length),
        evaluations, rejected, accepted [K], state (names), theta [K, p], loss [K] (of theta; NaN for a FAILED problem); launches; with a prior also prior_loss [K], the
        prior's share of loss"""
        acc = self.accepted.cpu().numpy()
        n = np.minimum(acc, self.loss_trace.shape[1])
        lt, pt, lmt = self.loss_trace.cpu().numpy(), self.parameter_trace.cpu().numpy(), self.lambda_trace.cpu().numpy()
        state = self.state.cpu().numpy()
        loss = np.where(acc > 0, self.current[:, self.p].cpu().numpy(), np.nan)
        r = {"loss_trace": [lt[k, :n[k]].copy() for k in range(self.K)], "parameter_trace": [pt[k, :n[k]].copy() for k in range(self.K)],
             "lambda_trace": [lmt[k, :n[k]].copy() for k in range(self.K)], "evaluations": self.evaluations.cpu().numpy(), "rejected": self.rejected.cpu().numpy(),
             "accepted": acc, "state": [rt.LM_STATES[v] for v in state], "theta": self.theta.cpu().numpy(), "loss": loss, "launches": self.launches}
        if self.prior_loss is not None:
            r["prior_loss"] = self.prior_loss.cpu().numpy()
        return r

    def covariance(self, noise="known", n_observed=None):
        """K error bars for K estimates, one launch (pdp_lm_covariance_batched) on `current` - G = J'J of the mean row at the accepted points (with a prior: J'J + P / S,
        the posterior precision).  noise="known": the weights are 1 / sigma^2, Cov = (S G)^-1.  noise="estimated": sigma^2_k = S loss_k / (N_k - p) scales it; N_k is
        the number of observed entries of problem k (n_observed [K], or what for_sysid / for_irl counted); N_k <= p gives NaN for that problem; with a prior it is a
        ValueError (the loss of the row contains the prior's share).  Returns host arrays: cov [K, p, p] (symmetrised (C + C') / 2), std_err [K, p], pivot_ratio [K]
        (smallest over largest pivot magnitude of the elimination: the diagnosis of a partially identifiable problem), status [K] (0, or 1 where G is singular to the
        elimination or not finite: NaN, pivot_ratio 0), sigma2 [K] (1 for "known").  Under Huber weights this is the covariance of the final reweighted least-squares
        problem, not the sandwich estimator."""
        torch = rt.torch_cuda()
        if noise not in ("known", "estimated"):
            raise ValueError("BatchedLMLoop.covariance: noise is 'known' or 'estimated'")
        S, p = float(self.S), self.p
        if noise == "estimated":
            if self.prior_mean is not None:
                raise ValueError("BatchedLMLoop.covariance: noise='estimated' with a prior - the loss of the row contains the prior's share; give the weights as "
                                 "1 / sigma^2 and use noise='known'")
            N = n_observed if n_observed is not None else self.n_observed
            if N is None:
                raise ValueError("BatchedLMLoop.covariance(noise='estimated'): the number of observed entries per problem is not known: give n_observed [K]")
            N = torch.as_tensor(N, device="cuda").to(torch.float64).reshape(-1).expand(self.K)
            sigma2 = torch.where(N > p, S * self.current[:, p] / (N - p), torch.full_like(N, float("nan")))
        else:
            sigma2 = torch.ones((self.K,), dtype=torch.float64, device="cuda")
        out = rt.lm_covariance(self.current, (sigma2 / S).contiguous())
        cov = 0.5 * (out["cov"] + out["cov"].transpose(1, 2))
        return {"cov": cov.cpu().numpy(), "std_err": out["std_err"].cpu().numpy(), "pivot_ratio": out["pivot_ratio"].cpu().numpy(), "status": out["status"].cpu().numpy(),
                "sigma2": sigma2.cpu().numpy()}

    @classmethod
    def for_sysid(cls, mdl, inputs, states, theta0, samples_per_problem=1, ini_state=None, skip_missing=False, estimate_ini=None, weights=None, huber_delta=None,
                  prior_ini_precision=None, **kw):
        """One SysID problem per group of samples_per_problem consecutive trajectories: inputs [K S, T, m], states [K S, T+1, n], theta0 [K, p] or [p].  An evaluation is
        ONE launch of mdl.sysid_step(gauss_newton=True) with the trial points as per-sample parameters; a sample is bad where its row holds a non-finite entry (formed on
        the device).  skip_missing, ini_state: as in LMLoop.for_sysid (a NaN in the initial state under skip_missing is a ValueError before any launch).
        estimate_ini (state indices or a bool mask [n]): one problem per TRAJECTORY (samples_per_problem == 1) whose vector is [theta_k | x0_k[idx]], W = p + q <= 16
        unknowns; theta0 is [p], [K, p] (the estimated components start from ini_state, or states[:, 0]) or [K, W].  An evaluation is one launch of
        pdp_sysid_step_gn_ini_batched: theta is read from the trial rows in place (row stride W), the estimated components are copied from the trial rows into a
        persistent x0 buffer at a fixed address - one small device copy, no host synchronisation; the update launch is pdp_lm_update_batched's with W as its p.
        loop.split(theta [K, W]) -> (theta [K, p], ini_state [K, n]).
        weights, huber_delta: as in LMLoop.for_sysid - checked once here, then every evaluation is one launch of pdp_sysid_step_wls_batched.
        prior_mean, prior_precision (keywords of the class, in natural units, on theta: [p] or [K, p]; [p], [K, p], [p, p] or [K, p, p]) pass through;
        prior_ini_precision [q] (with estimate_ini): a diagonal prior on the estimated components of x0, centred on their starting values - mean and precision are
        extended to the W = p + q vector.  The loop counts the observed entries per problem (covariance(noise="estimated")) by LMLoop.for_sysid's rule."""
        if prior_ini_precision is not None and not rt.ini_indices(estimate_ini, mdl.n)[0]:
            raise ValueError("BatchedLMLoop.for_sysid: prior_ini_precision needs estimate_ini")
        idx, _ = rt.ini_indices(estimate_ini, mdl.n)
        rows, held = mdl.sysid_rows_prepared(inputs, states, skip_missing, ini_state, idx, weights, huber_delta, own_x0=bool(idx), who="BatchedLMLoop.for_sysid",
                                             data_name="states")
        torch = rt.torch_cuda()

        def evaluate_rows(trial):                   # trial at a fixed address: [K S, p], or [K, W] = theta_k (read in place) | x0_k[idx] (copied into held["x0"])
            out = rows(trial)
            return out["packed_gn"], non_finite_rows(out["packed_gn"]).to(torch.int32)
        if idx:                                     # (nothing selected is estimate_ini=None; an estimated component still needs the finite starting value checked above)
            return cls._for_sysid_ini(mdl, evaluate_rows, held, theta0, samples_per_problem, ini_state, skip_missing, idx, weights=weights,
                                      prior_ini_precision=prior_ini_precision, **kw)
        inputs, states = held["u"], held["xobs"]
        B, T, S = int(inputs.shape[0]), int(inputs.shape[1]), int(samples_per_problem)
        assert states.shape == (B, T + 1, mdl.n) and inputs.shape == (B, T, mdl.m) and B % S == 0

        loop = cls(evaluate_rows, theta0, samples_per_problem=S, K=B // S, **kw)
        loop.n_observed = rt.count_observed(states, weights, skip_missing, _first_row(ini_state, None, mdl.n)).view(B // S, S).sum(dim=1)
        return loop

    @classmethod
    def _for_sysid_ini(cls, mdl, evaluate_rows, held, theta0, samples_per_problem, ini_state, skip_missing, idx, weights=None, prior_ini_precision=None,
                       prior_mean=None, prior_precision=None, prior_kind=None, **kw):
        torch = rt.torch_cuda()
        inputs, states, x0, cols = held["u"], held["xobs"], held["x0"], held["columns"]      # x0 persistent, at a fixed address
        K, T, p, q = int(inputs.shape[0]), int(inputs.shape[1]), mdl.p, len(idx)
        W = p + q
        assert states.shape == (K, T + 1, mdl.n) and inputs.shape == (K, T, mdl.m)
        if int(samples_per_problem) != 1:
            raise ValueError("BatchedLMLoop.for_sysid(estimate_ini=): one problem per trajectory (samples_per_problem == 1); one shared theta with an initial state "
                             "per recording is LMLoop.for_sysid(estimate_ini=)")
        if W > 16:
            raise ValueError("BatchedLMLoop.for_sysid(estimate_ini=): p + q = %d + %d > 16 unknowns per problem" % (p, q))
        ini0 = x0.cpu().numpy().copy()
        th = rt.dev(theta0)
        th = (th[None].expand(K, -1) if th.dim() == 1 else th).reshape(K, -1)
        if th.shape[1] == p:
            th = torch.cat([th, x0[:, cols]], dim=1)
        if th.shape[1] != W:
            raise ValueError("BatchedLMLoop.for_sysid(estimate_ini=): theta0 is [p], [K, p] or [K, p + q] = [%d, %d], got %s" % (K, W, tuple(th.shape)))

        def split(theta):
            v = np.asarray(theta.cpu() if hasattr(theta, "cpu") else theta, dtype=float).reshape(K, W)
            ini = ini0.copy()
            ini[:, idx] = v[:, p:]
            return v[:, :p].copy(), ini

        mean, prec = check_prior("BatchedLMLoop.for_sysid", prior_mean, prior_precision, p, K, prior_kind)
        mean, prec, prior_kind = _prior_with_ini("BatchedLMLoop.for_sysid", mean, prec, prior_ini_precision, p, q, ini0[:, idx], K=K, prior_kind=prior_kind)
        if mean is not None and prior_ini_precision is None:        # a prior on theta alone: the components of x0 get none
            mean, prec, prior_kind = _prior_with_ini("BatchedLMLoop.for_sysid", mean, prec, np.zeros(q), p, q, ini0[:, idx], K=K, prior_kind=prior_kind)
        loop = cls(evaluate_rows, th, samples_per_problem=1, K=K, prior_mean=mean, prior_precision=prec, prior_kind=prior_kind, **kw)
        loop.split = split
        loop.n_observed = rt.count_observed(states, weights, skip_missing, _first_row(ini_state, idx, mdl.n))
        return loop

    @classmethod
    def for_irl(cls, mdl, demo_x, demo_u, theta0, samples_per_problem=1, tol=1e-10, max_iter=300, ini_state=None, skip_missing=False, weights_state=None,
                weights_control=None, huber_delta=None, **kw):
        """One IRL problem per group of samples_per_problem consecutive demonstrations: demo_x [K S, T+1, n], demo_u [K S, T, m], theta0 [K, p] or [p].  An evaluation
        solves every demonstration's OC problem at its problem's trial point (oc_solve_ms with per-sample parameters: the first cold, later ones warm from COPIES of the
        last accepted solutions) and runs the fused unit once with gauss_newton=True.  A sample is bad under LMLoop.for_irl's three conditions: its solve did not
        converge, reported trouble, or the unit set a status bit.  After the update the accepted solutions are refreshed where the launch accepted the sample's problem
        (torch.where on accepted_now: no host decision).  skip_missing, ini_state: as in LMLoop.for_irl.
        weights_state, weights_control, huber_delta: as in LMLoop.for_irl - checked once here, then every evaluation's unit is one launch of pdp_oc_pdp_grad_wls_batched.
        prior_mean, prior_precision (keywords of the class, in natural units) pass through; the loop counts the observed entries per problem
        (covariance(noise="estimated")) by LMLoop.for_irl's rule."""
        if skip_missing:
            rt.refuse_nan_initial_state("BatchedLMLoop.for_irl", demo_x, ini_state, "demo_x")
        rows, held = mdl.oc_rows_prepared(demo_x, demo_u, skip_missing, weights_state, weights_control, huber_delta)
        torch = rt.torch_cuda()
        demo_x, demo_u = held["demo_x"], held["demo_u"]
        B, T, S = int(demo_u.shape[0]), int(demo_u.shape[1]), int(samples_per_problem)
        assert demo_x.shape == (B, T + 1, mdl.n) and demo_u.shape == (B, T, mdl.m) and B % S == 0
        x0 = (demo_x[:, 0] if ini_state is None else rt.dev(ini_state).reshape(B, mdl.n)).contiguous()
        sols = {"accepted": None, "trial": None}

        def evaluate_rows(trial):
            s = mdl.oc_solve_ms(x0, trial, T, tol=tol, max_iter=max_iter, warm=sols["accepted"])
            out = rows(s["control"], trial, x=s["state"], lam=s["costate"])
            sols["trial"] = (s["state"], s["control"], s["costate"])
            return out["packed_gn"], bad_irl_samples(s, out).to(torch.int32)

        loop = cls(evaluate_rows, theta0, samples_per_problem=S, K=B // S, **kw)
        loop.n_observed = (rt.count_observed(demo_x, weights_state, skip_missing, _first_row(ini_state, None, mdl.n)) +
                           rt.count_observed(demo_u, weights_control, skip_missing)).view(B // S, S).sum(dim=1)

        def keep_accepted():
            now = (loop.accepted_now != 0)[:, None, None]
            if sols["accepted"] is None:            # the first launch: every usable problem was accepted; a FAILED one keeps the cold start's all-zero point
                sols["accepted"] = tuple(torch.where(now, t, torch.zeros_like(t)) for t in sols["trial"])
            else:
                sols["accepted"] = tuple(torch.where(now, t, a) for t, a in zip(sols["trial"], sols["accepted"]))
        loop.after_update = keep_accepted
        return loop


class MatrixFreeLM:
    """Levenberg-Marquardt for ONE shared parameter theta [p] (p <= 512) of a PDP.SysID `sid`, on ANY residual of its rollouts written in torch, without ever forming
    the Gauss-Newton matrix: the models LMLoop.for_sysid has no route for - wide ones (the fused Gauss-Newton row is p <= 16) and any measurement function h(x).
    residual(state [B, T+1, n]) -> r (a tensor of any shape) is a pure torch function; its own J_h v / J_h' w come from torch.func.jvp / vjp.  One evaluation is a
    rollout (SysID.integrateDyn_batch from ini_state [B, n] under inputs [B, T, m]) plus r, with loss = sum r^2 / B.  A Gauss-Newton product G v = J' J v / B is
    rollout_jvp_batch -> J_h -> J_h' -> rollout_vjp_batch summed over the batch: two launches of the model library whatever p is.  The step solves
    (G + lam I) s = J' r / B by conjugate gradients, written in torch on the device, from s = 0 to a relative residual of cg_tol or cg_max iterations (None: 2 p).
    Plain lam I damping: matrix-free there is no diag G, so Marquardt's scaling (lm_step's lam diag G) is not available - scale the parameters where their
    magnitudes differ by orders.  The accept / reject / lam schedule and the keys of run() are LMLoop's, and `cg_iterations` (all inner iterations so far).
    Out of scope: per-recording initial states, priors, covariance, process groups, Huber.  MatrixFreeLM.for_cp builds the same loop for the policy of a
    PDP.ControlPlanning, with residual(state, control): the loop reaches its model through a small adapter (rollout, J v, J' w) whose default is the SysID one."""

    def __init__(self, sid, ini_state, inputs, theta0, residual, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, cg_tol=1e-8, cg_max=None):
        shape = lambda a: tuple(int(k) for k in (a.shape if hasattr(a, "shape") else np.shape(a)))
        p, su = int(sid.n_auxvar), shape(inputs)
        if len(su) != 3 or su[2] != sid.n_control or su[0] < 1 or su[1] < 1:
            raise ValueError("MatrixFreeLM: inputs must be [B, T, m] with m = %d and B, T >= 1, got %s" % (sid.n_control, su))
        if shape(ini_state) != (su[0], sid.n_state):
            raise ValueError("MatrixFreeLM: ini_state must be [B, n] = %s, got %s" % ((su[0], sid.n_state), shape(ini_state)))
        if int(np.prod(shape(theta0))) != p:
            raise ValueError("MatrixFreeLM: theta0 must be [p] with p = %d (one parameter shared by the batch), got %s" % (p, shape(theta0)))
        if p > 512:
            raise ValueError("MatrixFreeLM: p = %d is beyond the rollout's jvp / vjp kernels (p <= 512)" % p)
        if not callable(residual):
            raise ValueError("MatrixFreeLM: residual must be a function of the rollouts [B, T+1, n]")
        self.sid, self.x0, self.u = sid, rt.dev(ini_state), rt.dev(inputs)
        self._setup(_SysIDSweeps(sid, self.x0, self.u), su[0], p, theta0, residual, lam0, up, down, lam_min, lam_max, cg_tol, cg_max)

    def _setup(self, sweeps, B, p, theta0, residual, lam0, up, down, lam_min, lam_max, cg_tol, cg_max):
        """the loop's state; `sweeps` is what it reaches the model through: rollout(theta) -> the tuple of tensors the residual takes, jv(traj, theta, v) -> their
        tangents along v [p], jt(traj, theta, cotangents) -> J' of them, summed over the batch"""
        self.sweeps, self.residual, self.B, self.p = sweeps, residual, B, p
        self.theta = rt.dev(theta0).reshape(p).clone()
        self.lam, self.up, self.down, self.lam_min, self.lam_max = float(lam0), float(up), float(down), float(lam_min), float(lam_max)
        self.cg_tol, self.cg_max = float(cg_tol), int(2 * p if cg_max is None else cg_max)
        self.current = None                     # (loss, g = J'r / B, the rollout (a tuple), residual's vjp at it) at self.theta
        self.evaluations = self.rejected = self.cg_iterations = 0
        self.stalled = False
        self.loss_trace, self.parameter_trace, self.lambda_trace = [], [], []

    def _eval(self, theta):
        """(loss, g, x, vjp of the residual at x), or None where the loss is not finite"""
        import torch
        self.evaluations += 1
        with torch.no_grad():
            traj = self.sweeps.rollout(theta)
        r, back = torch.func.vjp(self.residual, *traj)
        loss = float((r.detach() ** 2).sum()) / self.B
        if not np.isfinite(loss):
            return None
        g = self._jt(traj, theta, back(r.detach()))
        return loss, g, traj, back

    def _jt(self, traj, theta, w):
        """J' of the rollout on the cotangents of what the residual takes, summed over the batch, / B"""
        return self.sweeps.jt(traj, theta, w) / self.B

    def gauss_newton_product(self, v):
        """G v = J' J v / B at the accepted point, v [p] on the device: rollout_jvp -> J_h -> J_h' -> rollout_vjp"""
        import torch
        if self.current is None:
            self.start()
        _, _, traj, back = self.current
        jv = torch.func.jvp(self.residual, traj, self.sweeps.jv(traj, self.theta, v))[1]
        return self._jt(traj, self.theta, back(jv.detach()))

    def _cg(self, g):
        """(G + lam I) s = g by conjugate gradients from s = 0"""
        s, r = g.new_zeros(g.shape), g.clone()
        d, rr = r.clone(), float(r @ r)
        stop = (self.cg_tol ** 2) * rr
        for _ in range(self.cg_max):
            if not rr > stop:
                break
            q = self.gauss_newton_product(d) + self.lam * d
            dq = float(d @ q)
            self.cg_iterations += 1
            if not dq > 0.0:                    # (a non-finite product, or no curvature left in fp64)
                break
            a = rr / dq
            s, r = s + a * d, r - a * q
            rr_new = float(r @ r)
            d, rr = r + (rr_new / rr) * d, rr_new
        return s

    def start(self):
        """the evaluation at theta0 (the first accepted point)"""
        r = self._eval(self.theta)
        if r is None:
            raise RuntimeError("MatrixFreeLM: the initial parameter could not be evaluated")
        self.current = r
        self._record()

    def _record(self):
        self.loss_trace.append(self.current[0])
        self.parameter_trace.append(self.theta.detach().cpu().numpy().copy())
        self.lambda_trace.append(self.lam)

    def step(self):
        """one trial: True if it was accepted"""
        import torch
        loss, g = self.current[:2]
        trial = self.theta - self._cg(g)
        if bool(torch.isfinite(trial).all()):
            r = self._eval(trial)
        else:
            r, self.evaluations = None, self.evaluations + 1        # (a trial that cannot be formed still counts against the budget)
        if r is not None and r[0] < loss:
            self.theta, self.current = trial, r
            self.lam = max(self.lam / self.down, self.lam_min)
            self._record()
            return True
        self.rejected += 1
        self.lam *= self.up
        return False

    def run(self, max_evals=50, loss_tol=0.0):
        if self.current is None:
            self.start()
        while self.evaluations < max_evals and self.current[0] > loss_tol:
            if self.lam > self.lam_max:
                self.stalled = True
                break
            self.step()
        return self.results()

    def results(self):
        """LMLoop.results()'s fields over the ACCEPTED points, and cg_iterations"""
        return {"loss_trace": np.array(self.loss_trace), "parameter_trace": np.array(self.parameter_trace).reshape(len(self.parameter_trace), self.p),
                "lambda_trace": np.array(self.lambda_trace), "evaluations": self.evaluations, "rejected": self.rejected, "stalled": self.stalled,
                "iterations": len(self.loss_trace), "cg_iterations": self.cg_iterations}

    @classmethod
    def for_sysid(cls, sid, inputs, states, theta0, ini_state=None, weights=None, skip_missing=False, **kw):
        """The recorded-state residual of the SysID drivers: r = sqrt(weights) (state - states) over inputs [B, T, m] and recorded states [B, T+1, n], rolled out from
        ini_state [B, n] (None: states[:, 0]).  weights ([n], [T+1, n] or [B, T+1, n], >= 0, 0 = not observed) and, with skip_missing, the NaN entries of `states` (not
        observed) are applied elementwise in torch.  With skip_missing a NaN in the initial state that would be used is a ValueError before any launch."""
        import torch
        shape = lambda a: tuple(int(k) for k in (a.shape if hasattr(a, "shape") else np.shape(a)))
        su = shape(inputs)
        if len(su) != 3 or shape(states) != (su[0], su[1] + 1, sid.n_state):
            raise ValueError("MatrixFreeLM.for_sysid: inputs must be [B, T, m] and states [B, T+1, n] with n = %d, got %s and %s" % (sid.n_state, su, shape(states)))
        if skip_missing:
            rt.refuse_nan_initial_state("MatrixFreeLM.for_sysid", states, ini_state, "states")
        xobs = rt.dev(states)
        scale = torch.ones_like(xobs)
        if weights is not None:
            w = rt.dev(weights)
            if tuple(w.shape) not in ((sid.n_state,), tuple(xobs.shape[1:]), tuple(xobs.shape)) or bool((w < 0).any()) or not bool(torch.isfinite(w).all()):
                raise ValueError("MatrixFreeLM.for_sysid: weights must be [n], [T+1, n] or [B, T+1, n], finite and >= 0, got %s" % (tuple(w.shape),))
            scale = scale * torch.sqrt(w)
        missing = torch.isnan(xobs)
        if bool(missing.any()):
            if not skip_missing:
                raise ValueError("MatrixFreeLM.for_sysid: `states` holds a NaN - pass skip_missing=True to treat NaN entries as not observed")
            scale = torch.where(missing, torch.zeros_like(scale), scale)
        x0 = (xobs[:, 0] if ini_state is None else rt.dev(ini_state)).contiguous().clone()
        target = torch.where(missing, torch.zeros_like(xobs), xobs)
        return cls(sid, x0, inputs, theta0, lambda state: (state - target) * scale, **kw)

    @classmethod
    def for_cp(cls, cp, ini_state, horizon, theta0, residual, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, cg_tol=1e-8, cg_max=None):
        """The same loop for the policy of a PDP.ControlPlanning `cp` (setPolyControl / setNeuralPolicy): ONE theta [p] shared by the rollouts from ini_state [B, n]
        over `horizon` steps, residual(state [B, T+1, n], control [B, T, m]) -> r written in torch - planning to waypoints, to a reference trajectory, to a terminal
        state.  One evaluation is one rollout (ControlPlanning.integrateSys_batch); a Gauss-Newton product is rollout_jvp_batch -> J_h -> J_h' -> rollout_vjp_batch,
        two sweeps on the saved rollout whatever p is (no size is refused: beyond the sweeps' limits both take their materialised routes).  Schedule, inner solve and
        the keys of run(): those of the class."""
        shape = lambda a: tuple(int(k) for k in (a.shape if hasattr(a, "shape") else np.shape(a)))
        if not hasattr(cp, "_policy"):
            raise ValueError("MatrixFreeLM.for_cp: set the control policy first (setPolyControl / setNeuralPolicy / init_step)")
        p, sx = int(cp.n_auxvar), shape(ini_state)
        if len(sx) != 2 or sx[1] != cp.n_state or sx[0] < 1:
            raise ValueError("MatrixFreeLM.for_cp: ini_state must be [B, n] with n = %d and B >= 1, got %s" % (cp.n_state, sx))
        if int(horizon) < 1:
            raise ValueError("MatrixFreeLM.for_cp: horizon must be at least 1, got %s" % (horizon,))
        if int(np.prod(shape(theta0))) != p:
            raise ValueError("MatrixFreeLM.for_cp: theta0 must be [p] with p = %d (one policy shared by the batch), got %s" % (p, shape(theta0)))
        if not callable(residual):
            raise ValueError("MatrixFreeLM.for_cp: residual must be a function of the rollouts (state [B, T+1, n], control [B, T, m])")
        loop = cls.__new__(cls)
        loop.cp, loop.x0, loop.horizon = cp, rt.dev(ini_state), int(horizon)
        loop._setup(_CPSweeps(cp, loop.x0, loop.horizon), sx[0], p, theta0, residual, lam0, up, down, lam_min, lam_max, cg_tol, cg_max)
        return loop


class _SysIDSweeps:
    """MatrixFreeLM's way to a PDP.SysID: the rollout under the recorded inputs, its tangent and its adjoint sweep (the residual takes the states)"""

    def __init__(self, sid, x0, u):
        self.sid, self.x0, self.u = sid, x0, u

    def rollout(self, theta):
        return (self.sid.integrateDyn_batch(self.x0, self.u, theta),)

    def jv(self, traj, theta, v):
        return (self.sid.rollout_jvp_batch(traj[0], self.u, theta, d_auxvar=v),)

    def jt(self, traj, theta, w):
        return self.sid.rollout_vjp_batch(traj[0], self.u, theta, w[0].detach().contiguous(), want_ini=False)["grad_theta"].sum(dim=0)


class _CPSweeps:
    """... and to a PDP.ControlPlanning: the rollout under its policy (the residual takes the states and the controls)"""

    def __init__(self, cp, x0, horizon):
        self.cp, self.x0, self.horizon = cp, x0, horizon

    def rollout(self, theta):
        x, u, _ = self.cp.integrateSys_batch(self.x0, self.horizon, theta)
        return x, u

    def jv(self, traj, theta, v):
        out = self.cp.rollout_jvp_batch(traj[0], traj[1], theta, d_auxvar=v)
        return out["d_state"], out["d_control"]

    def jt(self, traj, theta, w):
        gx, gu = (a.new_zeros(a.shape) if g is None else g.detach().contiguous() for a, g in zip(traj, w))
        return self.cp.rollout_vjp_batch(traj[0], theta, gx, gu, want_ini=False)["grad_theta"].sum(dim=0)
