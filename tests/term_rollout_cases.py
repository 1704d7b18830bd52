"""Inputs that the tests of the rollout with a terminal cost share (mpcb_rollout_term): the table of terminal references and the LQR
blocks of a batch of resolved configurations."""
import numpy as np

STRONG = (10.0, 1.0, 1.0)        # lqr(q, qdot, r): pqq ~ 456 -- every step of the plain inputs is solved by the fast path
WEAK = (0.001, 0.001, 1.0)       # ... a weight that leaves the interior point its share of the steps under tight bounds
AMPLITUDE = np.array([0.02] * 6 + [0.05] * 6)


def table(cfgs, seed):
    """x_ref[i, t] = [q_0; 0] + [0.02 (6) | 0.05 (6)] * sin(0.4 t + phase), one phase per simulation and entry from
    default_rng([seed, 99]): [B, Nsim, 12]."""
    B, S = len(cfgs), cfgs[0]["Nsim"]
    phase = np.random.default_rng([seed, 99]).uniform(0.0, 2.0 * np.pi, (B, 12))
    base = np.stack([np.concatenate([c["q0"], np.zeros(6)]) for c in cfgs])
    t = np.arange(S)[None, :, None]
    return np.ascontiguousarray(base[:, None, :] + AMPLITUDE[None, None, :] * np.sin(0.4 * t + phase[:, None, :]))


def lqr_blocks(cfgs, weights=STRONG):
    """The LQR blocks of each simulation's own model: [B, 6, 3] (pqq, pqv, pvv per joint)."""
    from robotic_mpc_amd import terminal

    return np.stack([terminal._lqr(np.asarray(c["wcv"], dtype=np.float64), float(c["dt"]), *weights)["blocks"] for c in cfgs])


def flat18(blocks):
    """[B, 6, 3] -> [B, 18] = pqq 6 | pqv 6 | pvv 6, as mpcb_rollout_term takes them."""
    return np.ascontiguousarray(np.transpose(blocks, (0, 2, 1)).reshape(len(blocks), 18))


def records(blocks, x_ref_t):
    """The step's records [B, 30] = pqq 6 | pqv 6 | pvv 6 | x_e 12 (mpcb_step_term) of one step."""
    return np.concatenate([flat18(blocks), x_ref_t], axis=1)
