"""Writes profiles/dense_qp_distances.txt: per case of tests/dense_qp_cases.py the oracle-vs-dense distance and the dense
solve's LU-vs-refined estimate (computed here, on the CPU), and the device-vs-dense distances of both engines where a dump of
tests/test_gpu_dense_qp.py is given (DENSE_QP_DUMP=<file> pytest -m gpu tests/test_gpu_dense_qp.py; then pass <file> here).
Prints the ORACLE_VS_DENSE table of tests/test_dense_qp.py as a literal.

    python tests/tools/dense_qp_profile.py [gpu_dump.json]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NOTES = """\
Replaced cases (the bound 10 x distance would exceed 1e-9, the parity bar):
  N20-default, xhat draws 120 .. 125: |oracle - certified| = 2.5e-9, 1.8e-10 (kept out: 1.8e-9 bound), 4.1e-9, 2.8e-10, 7.8e-14
  (one active bound only), 2.8e-7 -- the interior point stops with the active components mu / lambda off their bound, and
  these draws have multipliers of 1e-3 .. 3e-7.  Draw 126 (nine active bounds, smallest multiplier 1.3e-4) is the case.
Inactive cases: the first seed 7000 + 10 N + j of helpers.random_parameter_cfgs whose minimiser clears every bound by 0.05.
"""


def main():
    import dense_qp as dq
    import dense_qp_cases as dc
    from oracle import orc

    orc.build()
    gpu = json.load(open(sys.argv[1])) if len(sys.argv) > 1 else {}
    rows, table = [], {}
    for c in dc.all_cases():
        qp, o = dc.dense_qp(c), dc.oracle_solution(orc, c)
        if c["active"]:
            r = dq.certify(qp, o["dX"], o["dU"])
            dist, extra = r["distance"], "active %3d  min mult %.2e  min slack %.2e" % (r["n_active"], r["min_multiplier"], r["min_slack"])
        else:
            r = dc.dense_solution(c)
            dist = float(max(np.abs(r["dX"] - o["dX"]).max(), np.abs(r["dU"] - o["dU"]).max()))
            idx, lo, hi = qp.bounded()
            extra = "inactive    min slack %.2e" % np.minimum(r["w"][idx] - lo, hi - r["w"][idx]).min()
        table[c["id"]] = (dist, r["lu_vs_refined"])
        dev = "  ".join("%s %.2e" % (k, v) for k, v in sorted(gpu.get(c["id"], {}).items()))
        rows.append("%-16s N %3d  dt %-6g oracle-vs-dense %.2e  LU-vs-refined %.1e  bound %.1e  oracle iters %3d  %s\n%18s%s"
                    % (c["id"], c["N"], c["cfg"]["dt"], dist, r["lu_vs_refined"], dc.tolerance(table, c["id"]), o["iters"], extra,
                       "device-vs-dense (max over geometries): ", dev or "(not measured)"))
    with open(os.path.join(ROOT, "profiles", "dense_qp_distances.txt"), "w") as f:
        f.write("Distances to the dense KKT reference (tests/dense_qp.py), max-abs over the QP step (dX, dU).\n"
                "oracle-vs-dense and LU-vs-refined: CPU; device-vs-dense: MI355X, both engines of BatchController.\n"
                "bound = max(10 x oracle-vs-dense, 1e-12): what tests/test_dense_qp.py and tests/test_gpu_dense_qp.py assert.\n\n")
        f.write("\n".join(rows) + "\n\n" + NOTES)
    print("ORACLE_VS_DENSE = {")
    for k, (d, l) in table.items():
        print('    "%s": (%.2e, %.1e),' % (k, d, l))
    print("}")


if __name__ == "__main__":
    main()
