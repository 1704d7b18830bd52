"""The cases of the weight-sensitivity tests (tests/test_emulation_sensw.py on the CPU, tests/test_gpu_controller_sensw.py on the
device): the cases of tests/sens_cases.py, their dense references (tests/sensw_checks.py) and the check of the issue."""
import numpy as np

import dense_qp_cases as dc
import sens_cases as scs
import sensw_checks as sw

# every case the two test files use: the reference of each meets the condition of sensw_checks.bounds on all its rows, and
# test_emulation_sensw.py cross-checks each against central differences of the full dense solve once
CASES = ("N1-rand", "N3-rand", "N7-rand", "N9-rand", "N12-rand", "N20-rand", "N40-rand", "N80-rand", "N130-rand", "N20-ramp")

_REFS = {}


def reference(cid):
    """The dense weight Jacobian of the case's reset step, computed once per session and left unchanged."""
    if cid not in _REFS:
        c = scs.case(cid)
        X, U = dc.guess(c)
        _REFS[cid] = sw.dense_weight_jacobian(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"])
    return _REFS[cid]


def random_weights(cfg, rng, zero=None):
    """Weights for the set-weights tests: w_u and w_qddot within x0.5 ... x2 of the configuration's, task weights in [10, 100],
    task weight `zero` (if given) exactly 0."""
    th0 = sw.theta(cfg)
    th = np.concatenate([th0[:2] * rng.uniform(0.5, 2.0, 2), rng.uniform(10.0, 100.0, 5)])
    if zero is not None:
        th[2 + zero] = 0.0
    return th


def u0_bound(cid):
    """The bound on |u0 - dense| of a case: 10 x its committed solver-vs-dense distance, floor 1e-12 (dense_qp_cases.tolerance)."""
    return max(10.0 * scs.eps(cid), 1e-12)


def check_against(ref, eps_case, du0_dw, tag, cid, record=None):
    """One simulation's du0_dw [7, 6] against a dense reference, per weight row p:
    |du0_dw[p] - J[p]|_max <= b_p = 10 max(d_ref_p, eps(case) A_p), with b_p <= 1e-6 max_c |J[p][c]|.  Prints each figure before it
    asserts; returns the distances."""
    b = sw.bounds(ref, eps_case)
    d = sw.distances(ref, du0_dw)
    for p in range(sw.NWEIGHT):
        print(f"\n[sensw] {tag} {cid} row {p}: |dw - J| = {d[p]:.2e} (bound {b[p]:.1e}, d_ref {ref['d_ref'][p]:.1e}, "
              f"A {ref['A'][p]:.2e}, max |J| {ref['scale'][p]:.2e})", end="")
        if record is not None:
            record[(tag, cid, p)] = (d[p], b[p], ref["d_ref"][p], ref["A"][p], ref["scale"][p])
    print()
    assert np.isfinite(du0_dw).all(), (tag, cid)
    assert (d <= b).all(), (tag, cid, d, b)
    return d


def check(cid, du0_dw, tag, record=None):
    """du0_dw of the case's reset step under the bound of the issue; with a horizon of 1 the task rows are exactly zero."""
    if scs.case(cid)["N"] == 1:
        assert (np.asarray(du0_dw)[2:] == 0.0).all(), (tag, cid)        # zeros, not small numbers
    return check_against(reference(cid), scs.eps(cid), du0_dw, tag, cid, record)


def dump(path, measured):
    with open(path, "w") as f:
        for (tag, cid, p), v in sorted(measured.items()):
            f.write("%-30s %-14s row %d  distance %.2e  bound %.1e  d_ref %.1e  A %.2e  max|J| %.2e\n" % ((tag, cid, p) + tuple(v)))
