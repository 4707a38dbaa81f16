"""torch.autograd layer over the optimal-control solution: `oc_trajectory` maps the parameter theta of a PDP.OCSys to the optimal
(state, control) trajectory and is differentiable in theta, so that any scalar loss written in torch on the trajectory can be minimised with
`loss.backward()` and torch.optim:

    state, control = oc_trajectory(oc, ini_state, horizon, theta)        # theta: CUDA fp64, requires_grad
    loss = ((state[:, ::10, :2] - keyframes) ** 2).sum()
    loss.backward()                                                      # theta.grad = dL/dtheta through the OC solution

Forward: OCSys.ocSolver_batch (the reference's OCSys.ocSolver, PDP.py:121-220, for a batch).  Backward: the gradient of a scalar L(x, u) through the solution is
sum_t (dL/dx_t)' X_t + (dL/du_t)' U_t with X_t = dx_t/dtheta, U_t = du_t/dtheta the solution of the auxiliary control system (PDP.py:582-608) at the optimal
trajectory - one launch of the fused unit in its cotangent mode (OCSys.pdp_vjp_batch, PDP_OC_COTANGENT in include/pdp_hip.h): the sensitivities are contracted with
the incoming gradients on the chip and never written out.  With ini_grad=True the layer is differentiable in the initial state as well - the input of an MPC layer,
what a state estimator or an encoder in front of the controller trains through:

    state, control = oc_trajectory(oc, ini_state, horizon, theta, ini_grad=True)      # ini_state: CUDA fp64 [B, n], requires_grad
    loss = ((state[:, -1] - goal) ** 2).sum()
    loss.backward()                                                      # ini_state.grad = dL/dx_0 (and theta.grad where theta requires one)

dL/dx_0 comes from an adjoint sweep with the Riccati gains of the same backward launch (pdp_oc_sens_out.grad_x0 in include/pdp_hip.h).

`sysid_trajectory` is the same for the rollouts of a PDP.SysID: it maps (ini_state, theta) to the states of x_{t+1} = f(x_t, u_t, theta) for given inputs and is
differentiable in theta and ini_state - and, with input_grad=True, in the inputs - so that a loss that is not "state minus recorded state" - a bearing or camera
measurement h(x), a regulariser on the rollout, a learned term - trains the model's parameters and unknown initial states, and plans or refines inputs through the model:

    state = sysid_trajectory(sid, ini_state, inputs, theta)              # [B, T+1, n]; theta (and ini_state) CUDA fp64, requires_grad
    loss = ((torch.sin(state[:, :, 0]) - recorded_sin) ** 2).sum()
    loss.backward()                                                      # theta.grad, ini_state.grad

    state = sysid_trajectory(sid, ini_state, inputs, theta, input_grad=True)      # inputs: CUDA fp64, requires_grad
    loss = ((state[:, -1] - goal) ** 2).sum() + 0.01 * (inputs ** 2).sum()
    loss.backward()                                                      # inputs.grad (and theta.grad, ini_state.grad where they require one)

Forward mode works through sysid_trajectory as well: with torch.autograd.forward_ad dual tensors for theta, ini_state and (with input_grad=True) inputs, the tangent
of the rollout is one launch of the tangent sweep d_x[t+1] = F_t d_x[t] + E_t d_theta + G_t d_u[t] (SysID.rollout_jvp_batch, include/pdp_hip_sysid_jvp.h).
torch.func transforms are out of scope.

Forward: SysID.integrateDyn_batch.  Backward: the adjoint sweep lam_t = dL/dx_t + F_t' lam_{t+1}, dL/dtheta += E_t' lam_{t+1}, dL/dx_0 = lam_0 - and, with input_grad,
dL/du_t = G_t' lam_{t+1} - in one launch (SysID.rollout_vjp_batch, include/pdp_hip_sysid_vjp.h, include/pdp_hip_sysid_vjp_u.h).

Limits.  Both layers: first order only (backward is once_differentiable).  oc_trajectory: no gradient with respect to ini_state unless it is asked for (ini_grad=True;
without the keyword an ini_state that requires a gradient is refused); no finite state / control bounds (the
bounded solve goes through a log-barrier model whose KKT system is not the one the unit differentiates).  sysid_trajectory: the gradient with respect to the inputs on
request only (input_grad=True; without the keyword an `inputs` that requires a gradient is refused), and only THROUGH the dynamics; no models without parameters."""
import warnings

import torch
from torch.autograd.function import once_differentiable


class _OCTrajectory(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, oc, ini_state, horizon, info_out, solver_kwargs):
        with torch.no_grad():
            sol = oc.ocSolver_batch(ini_state, horizon, theta.detach().cpu().numpy(), **solver_kwargs)
        bad = int((~sol["converged"]).sum())
        if bad:
            warnings.warn("oc_trajectory: %d of %d OC solves did not converge (largest |grad| = %.3e); they are differentiated at their last iterate"
                          % (bad, sol["converged"].numel(), float(sol["grad_norm"][~sol["converged"]].max())), RuntimeWarning)
        info_out.update(sol)
        x, u, lam = sol["state"], sol["control"], sol["costate"]
        ctx.oc, ctx.shared = oc, theta.dim() == 1
        ctx.save_for_backward(x, u, lam, theta.detach())
        return x.clone(), u.clone()          # (the saved tensors stay as the solver left them whatever the caller does to the outputs)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_state, grad_control):
        x, u, lam, theta = ctx.saved_tensors
        gx = torch.zeros_like(x) if grad_state is None else grad_state.to(torch.float64).contiguous()
        gu = torch.zeros_like(u) if grad_control is None else grad_control.to(torch.float64).contiguous()
        out = ctx.oc.pdp_vjp_batch(u, theta, gx, gu, state_traj=x, costate_traj=lam)
        bad = int((out["status"] != 0).sum())
        if bad:
            warnings.warn("oc_trajectory: the Riccati sweep of the backward pass reported numerical trouble on %d trajectories (status bits of "
                          "pdp_oc_pdp_grad_batched, include/pdp_hip.h)" % bad, RuntimeWarning)
        g = out["grad"]
        return (g.sum(dim=0) if ctx.shared else g.clone()), None, None, None, None, None


class _OCTrajectoryIni(torch.autograd.Function):
    """_OCTrajectory with the initial state as an input of the function (oc_trajectory(..., ini_grad=True)): the same forward, and a backward that computes exactly
    the gradients that are needed - dL/dx_0 from the adjoint sweep behind the one launch that also gives dL/dtheta"""

    @staticmethod
    def forward(ctx, theta, ini_state, oc, horizon, info_out, solver_kwargs):
        out = _OCTrajectory.forward(ctx, theta, oc, ini_state.detach(), horizon, info_out, solver_kwargs)
        ctx.want_theta, ctx.want_ini = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_state, grad_control):
        x, u, lam, theta = ctx.saved_tensors
        gx = torch.zeros_like(x) if grad_state is None else grad_state.to(torch.float64).contiguous()
        gu = torch.zeros_like(u) if grad_control is None else grad_control.to(torch.float64).contiguous()
        out = ctx.oc.pdp_vjp_batch(u, theta, gx, gu, state_traj=x, costate_traj=lam, want_ini=ctx.want_ini)
        bad = int((out["status"] != 0).sum())
        if bad:
            warnings.warn("oc_trajectory: the Riccati sweep of the backward pass reported numerical trouble on %d trajectories (status bits of "
                          "pdp_oc_pdp_grad_batched, include/pdp_hip.h)" % bad, RuntimeWarning)
        g = None
        if ctx.want_theta:
            g = out["grad"].sum(dim=0) if ctx.shared else out["grad"].clone()
        return g, (out["grad_x0"].clone() if ctx.want_ini else None), None, None, None, None


def oc_trajectory(oc, ini_state, horizon, theta, return_info=False, ini_grad=False, **solver_kwargs):
    """Optimal trajectory of the PDP.OCSys `oc` from ini_state [B, n] over `horizon` steps at the parameter `theta`, differentiable in theta.
    theta: CUDA fp64 tensor, [p] (one parameter shared by the batch: theta.grad is the sum over the batch) or [B, p] (one per sample).
    Returns (state [B, T+1, n], control [B, T, m]) - with return_info=True also the solver's dict (cost, converged, iterations, ...).
    solver_kwargs go to OCSys.ocSolver_batch (tol, max_iter, u_init, warm_start, ...).  Samples that did not converge give one RuntimeWarning per call and are
    differentiated at their last iterate.
    ini_grad=True: differentiable in ini_state as well.  ini_state must then be a CUDA fp64 tensor [B, n]; when it requires a gradient it receives dL/dx_0 through the
    solution (state[:, 0]'s own cotangent included) from the one backward launch that also gives theta.grad.  A theta that requires no gradient is allowed then."""
    if not (torch.is_tensor(theta) and theta.is_cuda and theta.dtype == torch.float64):
        raise TypeError("oc_trajectory: theta must be a CUDA fp64 tensor ([p] shared, or [B, p] per sample)")
    if ini_grad:
        if not (torch.is_tensor(ini_state) and ini_state.is_cuda and ini_state.dtype == torch.float64 and ini_state.dim() == 2):
            raise TypeError("oc_trajectory: with ini_grad=True ini_state must be a CUDA fp64 tensor [B, n]")
    elif torch.is_tensor(ini_state) and ini_state.requires_grad:
        raise NotImplementedError("oc_trajectory: the gradient with respect to ini_state is not implemented (the auxiliary control system is solved with X_0 = 0); "
                                  "pass ini_state.detach()")
    if oc.has_bounds():
        raise NotImplementedError("oc_trajectory: finite state / control bounds are not supported - the bounded solve runs on a log-barrier model whose KKT system is "
                                  "not the one the gradient unit differentiates")
    if theta.dim() not in (1, 2) or theta.shape[-1] != oc.n_auxvar:
        raise ValueError("oc_trajectory: theta must be [p] or [B, p] with p = %d, got %s" % (oc.n_auxvar, tuple(theta.shape)))
    info = {}
    if ini_grad:
        if ini_state.shape[-1] != oc.n_state:
            raise ValueError("oc_trajectory: ini_state must be [B, n] with n = %d, got %s" % (oc.n_state, tuple(ini_state.shape)))
        state, control = _OCTrajectoryIni.apply(theta, ini_state, oc, int(horizon), info, solver_kwargs)
        return (state, control, info) if return_info else (state, control)
    x0 = ini_state.detach() if torch.is_tensor(ini_state) else ini_state
    state, control = _OCTrajectory.apply(theta, oc, x0, int(horizon), info, solver_kwargs)
    return (state, control, info) if return_info else (state, control)


class _SysIDTrajectory(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ini_state, inputs, sid, input_grad):
        with torch.no_grad():
            x = sid.integrateDyn_batch(ini_state.detach(), inputs.detach(), theta.detach())
        need = ctx.needs_input_grad
        # input_grad: exactly the outputs that are needed; without it the call the layer always made (grad_theta whatever theta requires)
        ctx.sid, ctx.shared, ctx.want_ini = sid, theta.dim() == 1, bool(need[1])
        ctx.want_theta, ctx.want_inputs = (bool(need[0]), bool(need[2])) if input_grad else (True, False)
        ctx.save_for_backward(x, inputs.detach(), theta.detach())
        ctx.save_for_forward(x, inputs.detach(), theta.detach())        # (what jvp reads: forward-mode differentiation)
        ctx.input_grad = bool(input_grad)
        ctx.set_materialize_grads(False)     # (jvp: an input without a tangent arrives as None, not as a tensor of zeros - a theta-only tangent does not pay for df/du)
        return x.clone()                     # (the saved rollout stays as the kernel wrote it whatever the caller does to the output)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_state):
        x, inputs, theta = ctx.saved_tensors
        g = (torch.zeros_like(x) if grad_state is None else grad_state).to(torch.float64).contiguous()
        out = ctx.sid.rollout_vjp_batch(x, inputs, theta, g, want_ini=ctx.want_ini, want_theta=ctx.want_theta, want_inputs=ctx.want_inputs)
        gt = out.get("grad_theta")
        if gt is not None and ctx.shared:
            gt = gt.sum(dim=0)
        return gt, out.get("grad_x0"), out.get("grad_u"), None, None

    @staticmethod
    def jvp(ctx, d_theta, d_ini_state, d_inputs, _sid, _input_grad):
        """forward mode (torch.autograd.forward_ad): the tangent of the rollout along the tangents of theta ([p] or [B, p]), ini_state and - with input_grad - inputs,
        None where an input carries none: one launch of the tangent sweep"""
        x, inputs, theta = ctx.saved_tensors
        if d_inputs is not None and not ctx.input_grad:
            raise NotImplementedError("sysid_trajectory: the tangent with respect to the inputs (through df/du) is computed on request only - pass input_grad=True")
        return ctx.sid.rollout_jvp_batch(x, inputs, theta, d_auxvar=d_theta, d_ini_state=d_ini_state, d_inputs=d_inputs)


def sysid_trajectory(sid, ini_state, inputs, theta, input_grad=False):
    """Rollouts of the PDP.SysID `sid` from ini_state [B, n] under inputs [B, T, m] at the parameter `theta`, differentiable in theta and ini_state: returns state
    [B, T+1, n].  theta: CUDA fp64 tensor, [p] (one parameter shared by the batch: theta.grad is the sum over the batch) or [B, p] (one per sample).  ini_state: an array
    or a tensor; a CUDA fp64 tensor that requires a gradient gets one (dL/dx_0, state[:, 0]'s own cotangent included).
    input_grad=True: differentiable in the inputs as well.  `inputs` must then be a CUDA fp64 tensor; when it requires a gradient it receives dL/dinputs THROUGH THE
    DYNAMICS (a loss that also uses `inputs` directly gets that term from torch as usual).  Backward computes exactly the gradients that are needed, all in one launch:
    a theta that does not require a gradient gets none computed."""
    if not (torch.is_tensor(theta) and theta.is_cuda and theta.dtype == torch.float64):
        raise TypeError("sysid_trajectory: theta must be a CUDA fp64 tensor ([p] shared, or [B, p] per sample)")
    if input_grad:
        if not (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float64):
            raise TypeError("sysid_trajectory: with input_grad=True the inputs must be a CUDA fp64 tensor [B, T, m]")
    elif torch.is_tensor(inputs) and inputs.requires_grad:
        raise NotImplementedError("sysid_trajectory: the gradient with respect to the inputs (through df/du) is computed on request only - pass input_grad=True, or "
                                  "inputs.detach()")
    if theta.dim() not in (1, 2) or theta.shape[-1] != sid.n_auxvar:
        raise ValueError("sysid_trajectory: theta must be [p] or [B, p] with p = %d, got %s" % (sid.n_auxvar, tuple(theta.shape)))
    if torch.is_tensor(ini_state) and ini_state.requires_grad and not (ini_state.is_cuda and ini_state.dtype == torch.float64):
        raise TypeError("sysid_trajectory: an ini_state that requires a gradient must be a CUDA fp64 tensor")
    from . import runtime
    x0, u = (ini_state if torch.is_tensor(ini_state) else runtime.dev(ini_state)), (inputs if input_grad else runtime.dev(inputs))
    return _SysIDTrajectory.apply(theta, x0, u, sid, bool(input_grad))


class _CPTrajectory(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ini_state, cp, horizon):
        with torch.no_grad():
            x, u, _ = cp.integrateSys_batch(ini_state.detach(), horizon, theta.detach())
        need = ctx.needs_input_grad
        ctx.cp, ctx.shared, ctx.want_theta, ctx.want_ini = cp, theta.dim() == 1, bool(need[0]), bool(need[1])
        ctx.save_for_backward(x, theta.detach())
        ctx.save_for_forward(x, u, theta.detach())                          # (what jvp reads: forward-mode differentiation takes the controls as given)
        ctx.set_materialize_grads(False)     # (and in jvp an input without a tangent arrives as None, not as a tensor of zeros)
        return x.clone(), u.clone()              # (the saved rollout stays as the kernel wrote it whatever the caller does to the output)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_state, grad_control):
        saved = ctx.saved_tensors
        x, theta = saved[0], saved[-1]
        B, T = x.shape[0], x.shape[1] - 1
        gx = (torch.zeros_like(x) if grad_state is None else grad_state).to(torch.float64).contiguous()
        gu = (x.new_zeros((B, T, ctx.cp.n_control)) if grad_control is None else grad_control).to(torch.float64).contiguous()
        out = ctx.cp.rollout_vjp_batch(x, theta, gx, gu, want_theta=ctx.want_theta, want_ini=ctx.want_ini)
        gt = out.get("grad_theta")
        if gt is not None and ctx.shared:
            gt = gt.sum(dim=0)
        return gt, out.get("grad_x0"), None, None

    @staticmethod
    def jvp(ctx, d_theta, d_ini_state, _cp, _horizon):
        """forward mode (torch.autograd.forward_ad): the tangents of (state, control) along the tangents of theta ([p] or [B, p]) and ini_state, None where an input
        carries none: one launch of the tangent sweep"""
        x, u, theta = ctx.saved_tensors
        out = ctx.cp.rollout_jvp_batch(x, u, theta, d_auxvar=d_theta, d_ini_state=d_ini_state)
        return out["d_state"], out["d_control"]


def cp_trajectory(cp, ini_state, horizon, theta):
    """Rollouts of the PDP.ControlPlanning `cp` from ini_state [B, n] over `horizon` steps under its policy u_t = pi(t, x_t, theta) (setPolyControl / setNeuralPolicy),
    differentiable in theta and ini_state: returns (state [B, T+1, n], control [B, T, m]).  Any scalar loss written in torch on them - a waypoint, an obstacle term, a
    learned critic, a terminal constraint - trains the policy with loss.backward(); ControlPlanning.step knows the model's own cost only.  theta: CUDA fp64 tensor, [p]
    (one policy shared by the batch: theta.grad is the sum over the batch) or [B, p] (one per sample).  ini_state: an array or a tensor; a CUDA fp64 tensor that
    requires a gradient gets one (dL/dx_0, state[:, 0]'s own cotangent included).  Forward: ControlPlanning.integrateSys_batch.  Backward: one launch of the adjoint
    sweep mu_t = dL/dx_t + F_t' mu_{t+1} + (d pi/dx)' v_t, v_t = dL/du_t + G_t' mu_{t+1}, dL/dtheta += (d pi/d theta)' v_t (ControlPlanning.rollout_vjp_batch,
    pdp_policy_cot in include/pdp_hip.h), which computes exactly the gradients that are needed; a missing cotangent is zeros.  Forward
    mode: with torch.autograd.forward_ad dual tensors for theta and / or ini_state the tangents of (state, control) are one launch of the tangent sweep
    du_t = pi_x dx_t + pi_theta d_theta, dx_{t+1} = F_t dx_t + G_t du_t on the saved rollout (ControlPlanning.rollout_jvp_batch, pdp_policy_tan in include/pdp_hip.h,
    DESIGN.md section 4.1p).  First order only; torch.func transforms are out of scope."""
    if not (torch.is_tensor(theta) and theta.is_cuda and theta.dtype == torch.float64):
        raise TypeError("cp_trajectory: theta must be a CUDA fp64 tensor ([p] shared, or [B, p] per sample)")
    if not hasattr(cp, "_policy"):
        raise ValueError("cp_trajectory: set the control policy first (setPolyControl / setNeuralPolicy / init_step)")
    if theta.dim() not in (1, 2) or theta.shape[-1] != cp.n_auxvar:
        raise ValueError("cp_trajectory: theta must be [p] or [B, p] with p = %d, got %s" % (cp.n_auxvar, tuple(theta.shape)))
    if torch.is_tensor(ini_state) and ini_state.requires_grad and not (ini_state.is_cuda and ini_state.dtype == torch.float64):
        raise TypeError("cp_trajectory: an ini_state that requires a gradient must be a CUDA fp64 tensor")
    if int(horizon) < 1:
        raise ValueError("cp_trajectory: horizon must be at least 1, got %s" % (horizon,))
    from . import runtime
    x0 = ini_state if torch.is_tensor(ini_state) else runtime.dev(ini_state)
    if x0.dim() != 2 or x0.shape[-1] != cp.n_state:
        raise ValueError("cp_trajectory: ini_state must be [B, n] with n = %d, got %s" % (cp.n_state, tuple(x0.shape)))
    if theta.dim() == 2 and theta.shape[0] != x0.shape[0]:
        raise ValueError("cp_trajectory: a per-sample theta must be [B, p] with B = %d, got %s" % (x0.shape[0], tuple(theta.shape)))
    return _CPTrajectory.apply(theta, x0, cp, int(horizon))
