#!/usr/bin/env python3
"""Learning the parameters of an optimal control system from SPARSE KEYFRAMES, with the OC solution as a torch.autograd layer.

The reference's IRL drivers (Examples/IRL/<sys>/<sys>_PDP.py) hard-wire one loss: the squared distance to a full demonstration, every state and every control of
every step.  Here only every tenth state of the cart-pole demonstrations is observed, and of it only the cart position and the pole angle - no velocities, no controls.
The loss is written in torch on the output of pdp_amd.autograd.oc_trajectory, `loss.backward()` differentiates through the OC solution (one launch of the fused unit
in its cotangent mode: the sensitivities dx/dtheta, du/dtheta are contracted with dL/dx, dL/du on the chip), and a torch.optim optimiser moves the parameters.

    python examples/oc_layer_custom_loss.py --iters 50 --lr 5e-3
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo                     # noqa: E402
from pdp_amd.autograd import oc_trajectory       # noqa: E402
from pdp_amd.sx import vertcat                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--batch", type=int, default=5, help="number of demonstrations used (at most the 5 stored ones)")
    ap.add_argument("--every", type=int, default=10, help="a keyframe every so many steps")
    ap.add_argument("--sigma", type=float, default=0.3, help="initial parameter = true + U(-sigma/2, sigma/2)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    env, dt = zoo.make_env("cartpole", "irl")
    oc = PDP.OCSys("cartpole")
    oc.setAuxvarVariable(vertcat(env.dyn_auxvar, env.cost_auxvar))
    oc.setControlVariable(env.U)
    oc.setStateVariable(env.X)
    oc.setDyn(env.X + dt * env.f)
    oc.setPathCost(env.path_cost)
    oc.setFinalCost(env.final_cost)

    d = np.load(os.path.join(ROOT, "examples", "data", "demos_cartpole.npz"))
    B = min(a.batch, d["state"].shape[0])
    T = d["control"].shape[1]
    x0 = d["state"][:B, 0]
    frames = list(range(a.every, T + 1, a.every))                                   # x_0 is given: no information in it
    keyframes = torch.as_tensor(d["state"][:B][:, frames, :2], device="cuda")       # cart position and pole angle only
    rng = np.random.default_rng(a.seed)
    true_parameter = d["true_parameter"]
    theta = torch.tensor(true_parameter + a.sigma * rng.random(true_parameter.size) - a.sigma / 2, dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([theta], lr=a.lr)
    loss_trace, warm = [], None
    t0 = time.time()
    for k in range(a.iters):
        opt.zero_grad()
        state, control, info = oc_trajectory(oc, x0, T, theta, return_info=True, warm_start=warm)
        warm = {key: info[key] for key in ("state", "control", "costate")}         # the next solve starts from this one
        loss = ((state[:, frames, :2] - keyframes) ** 2).sum()
        loss.backward()
        opt.step()
        loss_trace.append(float(loss))
        print("iter %5d  loss %.6e  |theta - theta*| %.4f" % (k, loss_trace[-1], float(np.abs(theta.detach().cpu().numpy() - true_parameter).max())))
    print("done: %d iterations x %d demonstrations, %d keyframes of 2 components each, in %.2f s  (loss %.4e -> %.4e)"
          % (a.iters, B, len(frames), time.time() - t0, loss_trace[0], loss_trace[-1]))
    return loss_trace


if __name__ == "__main__":
    main()
