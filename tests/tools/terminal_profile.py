"""Writes profiles/step_terminal_distances.txt: per case of tests/terminal_cases.py the oracle-vs-dense distance and the dense
solve's LU-vs-refined estimate of the terminal QP (computed here, on the CPU), and the distances of the emulated latency engine and
of both device engines where dumps of the tests are given (TERMINAL_DUMP=<file> pytest tests/test_terminal_cases.py
tests/test_terminal_sens.py, and TERMINAL_DUMP=<file> pytest -m gpu tests/test_gpu_terminal.py tests/test_gpu_terminal_sens.py; then
pass the files here).  Prints the ORACLE_VS_DENSE_TERM table of tests/test_terminal_cases.py as a literal.

    python tests/tools/terminal_profile.py [dump.json ...]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NOTES = """\
x_e: the guess's terminal state + uniform +-0.02 (q) / +-0.05 (qdot) from seed 500 + N; N = 135 takes seed 500 + N + 1000 x 28, the
  first whose bound-free minimiser clears every bound by 0.05 (the draws before it leave 0.02 or less, most of them active bounds).
N20-tight-term: as specified (dense_qp_cases.TIGHT, xhat seed 120) NO bound is active -- this terminal cost holds the terminal
  velocities at x_e and keeps every input 0.26 inside its bound; at every xhat seed 120 .. 519 the bound-free minimiser clears every
  bound by >= 0.068.  It is held to its certificate with n_active == 0.  N20-tight-far-term (the q offsets of x_e ten times as
  large) has five active bounds, multipliers >= 3.9e-2, free slack 1.1e-2.
Sensitivity rows (<case>-sens, N20-carried-sens): max-abs distance of du0_dx, du0_dyref and du0_dxe from central differences of
  the dense KKT solve; it equals the reference's own noise (the disagreement of its two step sizes, 1e-13 .. 2.4e-13).
"""


def main():
    import dense_qp as dq
    import dense_qp_cases as dc
    import terminal_cases as tc
    from oracle import orc

    orc.build()
    meas = {}
    for path in sys.argv[1:]:
        for cid, d in json.load(open(path)).items():
            for tag, v in d.items():
                meas.setdefault(cid, {})[tag] = max(v, meas.get(cid, {}).get(tag, 0.0))
    rows, table = [], {}
    for c in tc.all_cases():
        o = tc.oracle_solution(orc, c)
        dist, r = tc.distance(c, o["dX"], o["dU"])
        if c["certify"]:
            extra = "active %3d  min mult %.2e  min slack %.2e" % (r["n_active"], r["min_multiplier"], r["min_slack"])
        else:
            X, U = dc.guess(c)
            plain = dq.solve_equality(dq.assemble(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"]))
            extra = "inactive    clearance %.2e  |u0 - u0 without terminal cost| %.2e" % (tc.clearance(c), np.abs(r["dU"][0] - plain["dU"][0]).max())
        table[c["id"]] = (dist, r["lu_vs_refined"])
        m = "  ".join("%s %.2e" % (k, v) for k, v in sorted(meas.get(c["id"], {}).items()) if k != "oracle")
        rows.append("%-24s N %3d  dt %-6g oracle-vs-dense %.2e  LU-vs-refined %.1e  bound %.1e  oracle iters %3d  %s\n%18s%s"
                    % (c["id"], c["N"], c["cfg"]["dt"], dist, r["lu_vs_refined"], tc.tolerance(table, c["id"]), o["iters"], extra,
                       "engine-vs-dense: ", m or "(not measured)"))
    other = ["%-24s %s" % (cid, "  ".join("%s %.2e" % kv for kv in sorted(d.items()))) for cid, d in sorted(meas.items()) if cid not in table]
    with open(os.path.join(ROOT, "profiles", "step_terminal_distances.txt"), "w") as f:
        f.write("Controller step with a joint-wise terminal cost (mpcb_step_term): distances to the dense KKT reference of the terminal QP\n"
                "(tests/dense_qp_terminal.py), max-abs over the QP step (dX, dU).  oracle-vs-dense and LU-vs-refined: CPU; emu-*: the\n"
                "emulated latency engine (wavefronts, pool); latency* / stream*: MI355X, both engines of BatchController, forced geometries\n"
                "-w<wavefronts>_s<simulations per CU>.  bound = max(10 x oracle-vs-dense, 1e-12): what the tests assert.\n\n")
        f.write("\n".join(rows) + "\n\nChained steps and sensitivities:\n" + "\n".join(other) + "\n\n" + NOTES)
    print("ORACLE_VS_DENSE_TERM = {")
    for k, (d, l) in table.items():
        print('    "%s": (%.2e, %.1e),' % (k, d, l))
    print("}")


if __name__ == "__main__":
    main()
