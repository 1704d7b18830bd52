"""Writes profiles/dense_sqp_distances.txt: per case of tests/dense_sqp_cases.py and per SQP iteration the step length, the number
of active bounds, the dense residual norms, the oracle's distances to the dense replay (computed here, on the CPU) and the
device's where a dump of tests/test_gpu_dense_sqp.py is given (DENSE_SQP_DUMP=<file> pytest -m gpu tests/test_gpu_dense_sqp.py;
then pass <file> here).  Prints the ORACLE_VS_DENSE_SQP table of tests/test_dense_sqp.py and the WANT table of
tests/dense_sqp_cases.py as literals.

    python tests/tools/dense_sqp_profile.py [gpu_dump.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

NOTES = """\
Seeds: helpers.random_parameter_cfgs draws with the feedback state +-0.3 rad / +-1 rad/s off the packed start, scanned on the CPU
(oracle iterates, dense replay at qp_tol 1e-12).  Most draws take full steps and converge within two to four iterations, where the
merit decrease falls below 1e-6 |m0| and the replay refuses the case; the ones kept backtrack with every merit decision at least
1e-6 |m0| clear.
Replaced (the bound 10 x distance would exceed 1e-9): N = 12 seed 17 with the packed reference (7.4e-10; kept under the ramp
reference, 8.8e-12), seed 23 under the ramp (6.2e-10), seeds 250, 346, 454, 470, 642, 665, 778 (active, 6e-10 .. 2e-8);
N = 128 seeds 28 (2.9e-8) and 17 (3.1e-10).  N12-converges: seeds 0 .. 650 scanned, 184 is the first all-inactive draw that
converges with every merit decision and residual clear of its threshold.
"""
NAMES = ("cert", "res_stat", "res_eq", "res_ineq", "res_comp")


def main():
    import dense_sqp as ds
    import dense_sqp_cases as sc
    from oracle import orc

    orc.build()
    gpu = json.load(open(sys.argv[1])) if len(sys.argv) > 1 else {}
    out, table, want = [], {}, {}
    for c in sc.all_cases():
        rows = ds.replay(c, *sc.oracle_runs(orc, c))
        d = sc.distances(rows)
        table[c["id"]] = d
        w = {}
        al = {i: r["alpha"] for i, r in enumerate(rows) if not r["converged"] and r["alpha"] != 1.0}
        if al:
            w["alphas"] = al
        act = [i for i, r in enumerate(rows) if r["n_active"] > 0]
        if act:
            w["active_at"] = act
        else:
            w["inactive"] = True
        conv = [i for i, r in enumerate(rows) if r["converged"]]
        if conv:
            w["converges"] = conv[0]
        dfc = [i for i, r in enumerate(rows) if not r["converged"] and i > 0 and rows[i - 1]["alpha"] != 1.0 and r["defect"] > 1e-3 and i - 1 == 0]
        if dfc:
            w["defect_at"] = dfc
        want[c["id"]] = w
        out.append("%s  N %d  dt %g  M %d  fast path %s%s" % (c["id"], c["N"], c["cfg"]["dt"], c["M"], "on" if c["fast"] else "off",
                                                              "  ramp reference" if c["yref"] is not None else ""))
        for it, (r, dist) in enumerate(zip(rows, d)):
            head = "  it %d  converged" % it if r["converged"] else \
                "  it %d  alpha %-6.4g active %3d  merit margin %.1e  |b|,|dx0| %.1e" % (it, r["alpha"], r["n_active"], r["merit_margin"], r["defect"])
            out.append(head + "  dense residuals " + " ".join("%.3e" % v for v in r["dense_res"]))
            out.append("        oracle-vs-dense  " + "  ".join("%s %.2e" % (n, v) for n, v in zip(NAMES, dist)))
            out.append("        bound            " + "  ".join("%s %.1e" % (n, sc.tolerance(table, c["id"], it, k)) for k, n in enumerate(NAMES)))
            for tag, runs in sorted(gpu.get(c["id"], {}).items()):
                out.append("        %-16s " % tag + "  ".join("%s %.2e" % (n, v) for n, v in zip(NAMES, runs[it])))
        if c["id"] not in gpu:
            out.append("        device-vs-dense: (not measured)")
        out.append("")
    with open(os.path.join(ROOT, "profiles", "dense_sqp_distances.txt"), "w") as f:
        f.write("Distances of the full-SQP outer loop to the dense replay (tests/dense_sqp.py), per case and SQP iteration:\n"
                "cert = max-abs distance of the QP step / alpha to the certified dense solution; res_* = |reported - dense| of the four\n"
                "KKT residual norms the iteration's convergence test saw.  oracle-vs-dense: CPU; the other rows: MI355X, BatchController\n"
                "per engine and forced latency geometry (max over the runs of that tag).\n"
                "bound = max(10 x oracle-vs-dense, 1e-12): what tests/test_dense_sqp.py and tests/test_gpu_dense_sqp.py assert.\n\n")
        f.write("\n".join(out) + "\n" + NOTES)

    def lit(a):
        return {0.7: "A1", 0.7 * 0.7: "A2", 0.7 * 0.7 * 0.7: "A3"}.get(a, repr(a))

    print("WANT = {")
    for k, w in want.items():
        items = []
        for kk, v in w.items():
            items.append('"%s": %s' % (kk, "{" + ", ".join("%d: %s" % (i, lit(a)) for i, a in v.items()) + "}" if kk == "alphas" else repr(v)))
        print('    "%s": {%s},' % (k, ", ".join(items)))
    print("}")
    print("ORACLE_VS_DENSE_SQP = {")
    for k, d in table.items():
        print('    "%s": [' % k)
        for row in d:
            print("        (" + ", ".join("%.2e" % v for v in row) + "),")
        print("    ],")
    print("}")


if __name__ == "__main__":
    main()
