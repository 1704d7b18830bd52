"""The closed loop of the input-disturbance tests: a controller over a torch exact-ZOH plant with a constant input disturbance, run
nominal, disturbed without compensation, and disturbed with DisturbanceObserver feeding step(dist=d_hat).  Shared by the CPU
measurement on the emulated latency engine (tests/test_step_dist_closed_loop.py) and the device test (tests/test_gpu_step_dist.py):
the loop, the plant and the figures are the same code, only `step` differs.

N = 10, 4 simulations of config.base_params (they differ in d alone: uniform +-0.1, seed 970), pole = 0.2, 3 K steps where K is the
first step count with max_j ||(A - L C)_j^K||_2 <= 1e-8.
"""
import numpy as np

import dense_qp as dq
import dense_qp_cases as dc

N, B, POLE, D_SEED = 10, 4, 0.2, 970
# max |e_comp - e_nom| / max |e_unc - e_nom| over the last third of the run, measured with the emulated latency engine on the CPU
# (tests/test_step_dist_closed_loop.py prints it; profiles/step_dist_closed_loop.txt), and the bound the device is held to: 10 x that
RHO_EMULATED = 0.131
RHO = 10.0 * RHO_EMULATED


def raw_config():
    return dc._base(N)


def disturbance():
    return np.random.default_rng(D_SEED).uniform(-0.1, 0.1, (B, 6))


def settle_steps(obs):
    """K: the first k with ||(A - L C)^k||_2 <= 1e-8 for every joint."""
    M = obs.error_matrix().cpu().numpy().reshape(-1, 2, 2)
    P = M.copy()
    for k in range(1, 1000):
        if max(np.linalg.norm(p, 2) for p in P) <= 1e-8:
            return k
        P = P @ M
    raise AssertionError("the observer's error dynamics do not settle")


def run(step, cfg, chain, d_plant, steps, observer=None, device="cpu"):
    """`step(x [B, 12] tensor, d_hat [B, 6] tensor or None) -> (u0 [B, 6], x_pred1 [B, 12])` tensors on `device`.  The plant is the
    exact discretisation of the model with the constant input disturbance d_plant.  Returns dict(e [steps, B, 5] task errors of the
    plant states the controller saw, d_hat [steps, B, 6] or None, pred_err [steps, B]: max |x_pred1 - next plant state|)."""
    import torch

    A, Bm = (torch.from_numpy(m).to(device) for m in dq.lti(cfg["wcv"], cfg["dt"]))
    d = torch.from_numpy(np.ascontiguousarray(d_plant)).to(device)
    x = torch.from_numpy(np.tile(np.concatenate([cfg["q0"], cfg["qdot0"]]), (B, 1))).to(device)
    u_prev = torch.zeros((B, 6), dtype=torch.float64, device=device)
    ref = dq.packed_reference(cfg)
    e, dh, pe = [], [], []
    for _ in range(steps):
        d_hat = observer.update(x, u_prev) if observer is not None else None
        u0, xp1 = step(x, d_hat)
        u_prev = u0.clone()
        xn = x @ A.T + (u_prev + d) @ Bm.T
        xs = x.cpu().numpy()
        e.append(np.stack([dq.task_outputs(chain, cfg["coeffs"], cfg["t_ee"], xs[i]) - ref for i in range(B)]))
        dh.append(None if d_hat is None else d_hat.cpu().numpy().copy())
        pe.append((xp1 - xn).abs().amax(dim=1).cpu().numpy())
        x = xn
    return dict(e=np.stack(e), d_hat=None if observer is None else np.stack(dh), pred_err=np.stack(pe))


def three_runs(make_step, device="cpu"):
    """make_step() -> a fresh controller's `step` (see run).  Returns (K, nominal, uncompensated, compensated, d)."""
    from robotic_mpc_amd import config
    from robotic_mpc_amd.observer import DisturbanceObserver

    cfg = config.resolve_config(raw_config())
    chain = dc.chain_of(dict(cfg=cfg))
    d = disturbance()
    obs = DisturbanceObserver(np.asarray(cfg["wcv"], float), cfg["dt"], pole=POLE)
    K = settle_steps(obs)
    steps = 3 * K
    nom = run(make_step(), cfg, chain, np.zeros((B, 6)), steps, device=device)
    unc = run(make_step(), cfg, chain, d, steps, device=device)
    if device != "cpu":
        import torch

        obs = DisturbanceObserver(torch.as_tensor(np.asarray(cfg["wcv"], float), device=device), cfg["dt"], pole=POLE)
    comp = run(make_step(), cfg, chain, d, steps, observer=obs, device=device)
    return K, nom, unc, comp, d


def figures(K, nom, unc, comp, d):
    """dict(d_err: max |d_hat - d| from step K on; pred_comp: max |x_pred1 - next state| of the compensated run from step K + 1 on;
    pred_unc: the smallest such error of the uncompensated run over those steps; dev_comp / dev_unc: max |e - e_nom| over the last
    third; ratio)."""
    steps = nom["e"].shape[0]
    last = slice(steps - steps // 3, steps)
    dev_comp = float(np.abs(comp["e"][last] - nom["e"][last]).max())
    dev_unc = float(np.abs(unc["e"][last] - nom["e"][last]).max())
    return dict(d_err=float(np.abs(comp["d_hat"][K:] - d[None]).max()), pred_comp=float(comp["pred_err"][K + 1:].max()),
                pred_unc=float(unc["pred_err"][K + 1:].min()), dev_comp=dev_comp, dev_unc=dev_unc, ratio=dev_comp / dev_unc)
