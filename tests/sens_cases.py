"""The cases of the sensitivity tests (tests/test_emulation_sens.py on the CPU, tests/test_gpu_controller_sens.py on the device):
cases of tests/dense_qp_cases.py, and two more horizons built with its helpers."""
import numpy as np

import dense_qp_cases as dc
import sens_checks as sc
from test_dense_qp import BY_ID, CHAINED_ORACLE_VS_DENSE, ORACLE_VS_DENSE

# horizons dense_qp_cases has no case for, seeds by its rule (the first of 7000 + 10 N, + 1, ... whose minimiser clears every bound)
EXTRA = {9: 7090, 12: 7120, 30: 7300, 40: 7401}
_EXTRA = {}
# a case outside the committed table is held to the worst committed distance of the table's bound-inactive fast-path cases
EPS_WORST = max(v[0] for k, v in ORACLE_VS_DENSE.items() if k in BY_ID and BY_ID[k]["fast"] and not BY_ID[k]["active"])


def case(cid):
    if cid in BY_ID:
        return BY_ID[cid]
    N = int(cid[1:].split("-")[0])
    if cid not in _EXTRA:
        _EXTRA[cid] = dc.random_case(N, EXTRA[N])
        assert _EXTRA[cid]["id"] == cid
    return _EXTRA[cid]


def eps(cid):
    return ORACLE_VS_DENSE[cid][0] if cid in ORACLE_VS_DENSE else EPS_WORST


_REFS = {}


def reference(cid):
    """The dense Jacobians of the case's reset step, computed once per session and left unchanged."""
    if cid not in _REFS:
        c = case(cid)
        X, U = dc.guess(c)
        _REFS[cid] = sc.dense_jacobians(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"])
    return _REFS[cid]


def check(cid, du0_dx, du0_dyref, tag, record=None):
    """One simulation's sensitivities against the dense reference of its case, under the bound of the issue:
    10 x max(the reference's noise, the case's committed distance x max |J|) <= 1e-6 max |J|.  Returns the distance."""
    ref, N = reference(cid), case(cid)["N"]
    b = sc.bound(ref, eps(cid))
    d = sc.distance(ref, du0_dx, du0_dyref, N)
    print(f"\n[sens] {tag} {cid}: |J - J_dense| = {d:.2e} (bound {b:.1e}, d_ref {ref['d_ref']:.1e}, max |J| {ref['scale']:.2e})")
    if record is not None:
        record[(tag, cid)] = (d, b, ref["d_ref"], ref["scale"])
    assert np.isfinite(du0_dx).all() and np.isfinite(du0_dyref[:N]).all(), (tag, cid)
    assert d <= b, (tag, cid, d, b)
    assert (du0_dyref[0] == 0.0).all(), (tag, cid)                  # x_0 is pinned to xhat: exactly zero, not small
    assert (du0_dyref[N:] == 0.0).all(), (tag, cid)                 # rows past the simulation's own horizon (ragged batches)
    return d
