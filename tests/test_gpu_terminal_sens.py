"""BatchController.step(sens=True) with a terminal cost in force on the device (mpcb_step_term with sens, both engines): du0_dx,
du0_dyref and du0_dxe against central differences of the dense KKT solve of the terminal QP, under the bounds of
tests/test_terminal_sens.py: reset steps at N = 1, 2, 7, 20 and a stage-varying iterate, at the default geometry and at the forced
latency geometries (1, 1), (2, 1), (4, 1), (8, 2) and (4, 2) as mpcb_setup picks it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import terminal_cases as tc  # noqa: E402
from test_boundaries import PICKED_4_2, geo_name  # noqa: E402
from test_gpu_terminal import _clean, controller, numpy_step  # noqa: E402
from test_terminal_cases import BY_ID, CHAINED_ORACLE_VS_DENSE_TERM, ORACLE_VS_DENSE_TERM  # noqa: E402
from test_terminal_sens import RESET_HORIZONS, check_sens, reset_reference, stage_varying  # noqa: E402

pytestmark = pytest.mark.gpu

GEOS = [("stream", None), ("latency", None), ("latency", (1, 1)), ("latency", (4, 1)), ("latency", (8, 2)), ("latency", (2, 1)),
        ("latency", PICKED_4_2)]
IDS = ["%s%s" % (e, "" if g is None else "-" + geo_name(g)) for e, g in GEOS]


@pytest.mark.parametrize("engine,geo", GEOS, ids=IDS)
@pytest.mark.parametrize("N", RESET_HORIZONS)
def test_reset_step_sensitivities_against_dense(monkeypatch, engine, geo, N):
    _clean(monkeypatch, geo)
    cid = f"N{N}-rand-term"
    c = BY_ID[cid]
    ctl = controller([c], engine)
    out = numpy_step(ctl, c["xhat"][None], sens=True)
    ctl.close()
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1
    check_sens(reset_reference(cid), out, 0, ORACLE_VS_DENSE_TERM[cid][0], IDS[GEOS.index((engine, geo))], cid)
    if N == 1:
        assert (out["du0_dyref"][0] == 0.0).all() and np.abs(out["du0_dxe"][0]).max() > 1.0


@pytest.mark.parametrize("engine,geo", GEOS, ids=IDS)
def test_stage_varying_iterate_sensitivities_against_dense(monkeypatch, engine, geo):
    _clean(monkeypatch, geo)
    case = BY_ID[tc.CHAINED_CASE]
    ctl = controller([case], engine)
    ref, out = stage_varying(case, lambda x, sens: numpy_step(ctl, x[None], predict=True, sens=sens))
    ctl.close()
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1
    check_sens(ref, out, 0, max(CHAINED_ORACLE_VS_DENSE_TERM[False]), IDS[GEOS.index((engine, geo))], "N20-carried")


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_no_sensitivities_through_the_interior_point_and_ragged_rows(monkeypatch, engine):
    _clean(monkeypatch)
    cases = [BY_ID["N20-rand-term"], BY_ID["N20-rand-term-ipm"]]
    ctl = controller(cases, engine)
    out = numpy_step(ctl, np.stack([c["xhat"] for c in cases]), sens=True)
    ctl.close()
    assert list(out["sens_valid"]) == [1, 0]
    assert np.isfinite(out["du0_dxe"][0]).all() and np.isnan(out["du0_dxe"][1]).all() and np.isnan(out["du0_dx"][1]).all()
    check_sens(reset_reference("N20-rand-term"), out, 0, ORACLE_VS_DENSE_TERM["N20-rand-term"][0], engine + "-batch", "N20-rand-term")
