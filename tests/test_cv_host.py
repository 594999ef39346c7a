"""Public surface of renormalizer_amd.cv and the fixtures of its GPU tests (no GPU needed)."""
import inspect
import os
import re

import numpy as np

from renormalizer_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# parameter names and defaults of the reference (cv/spectra_cv.py:55-66, cv/zerot.py:55-68, cv/spectra_cv.py:17)
CV_PARAMS = [("model", None), ("spectratype", None), ("m_max", None), ("eta", None), ("h_mpo", None),
             ("method", "1site"), ("procedure_cv", None), ("rtol", 1e-5), ("b_mps", None), ("e0", None),
             ("cv_mps", None)]
ZT_PARAMS = CV_PARAMS + [("procedure_gs", None)]
BATCH_PARAMS = [("freq_reg", None), ("cores", None), ("obj", None), ("filename", None)]
REQUIRED = {"model", "spectratype", "m_max", "eta", "freq_reg", "cores", "obj"}


def _check_signature(fn, expected, skip_self):
    params = list(inspect.signature(fn).parameters.values())
    if skip_self:
        params = params[1:]
    assert [p.name for p in params] == [n for n, _ in expected]
    for p, (name, default) in zip(params, expected):
        if name in REQUIRED:
            assert p.default is inspect.Parameter.empty, name
        else:
            assert p.default == default, name


def test_cv_exports_and_signatures():
    import renormalizer_amd.cv as cv
    from renormalizer_amd.cv.spectra_cv import SpectraCv, batch_run
    from renormalizer_amd.cv.zerot import SpectraZtCV
    assert cv.SpectraZtCV is SpectraZtCV and cv.SpectraCv is SpectraCv and cv.batch_run is batch_run
    assert issubclass(SpectraZtCV, SpectraCv)
    _check_signature(SpectraCv.__init__, CV_PARAMS, True)
    _check_signature(SpectraZtCV.__init__, ZT_PARAMS, True)
    _check_signature(batch_run, BATCH_PARAMS, False)
    for name in ("cv_solve", "clear_res", "init_b_mps", "init_cv_mps", "oper_prepare", "optimize_cv", "initialize_LR",
                 "update_LR"):
        assert callable(getattr(SpectraZtCV, name)), name


def test_pcg_symbols_declared():
    for sym in ("mpse_pcg", "mpse_pcg_stats"):
        assert sym in E.EXPORTED_SYMBOLS
    header = open(os.path.join(REPO, "include", "mpsengine.h")).read()
    assert re.search(r"\bint\s+mpse_pcg\s*\(\s*mpse_ctx\s*\*\s*ctx,\s*int dtype,\s*const mpse_heff\s*\*\s*h,\s*int twolayer,"
                     r"\s*double shift,", header)
    assert re.search(r"\bint\s+mpse_pcg_stats\s*\(\s*mpse_ctx\s*\*\s*ctx,\s*int64_t\s*\*\s*counts,\s*int n\)", header)
    assert len(E._SIGNATURES["mpse_pcg"]) == 14 and len(E.Engine.PCG_STATS) == 10 and E.Engine.PCG_STATS[9] == "wait_interval"


def test_cv_fixtures(golden_dir):
    a = np.load(os.path.join(golden_dir, "cv_abs_zt.npy"))
    e = np.load(os.path.join(golden_dir, "cv_emi_zt.npy"))
    # recorded over np.arange(0.05, 0.11, 5e-5) and np.arange(-0.11, -0.05, 5e-5)
    assert a.shape == (1200, 1, 1) and e.shape == (1200,)
    assert len(np.arange(0.05, 0.11, 5e-5)) == 1200 and len(np.arange(-0.11, -0.05, 5e-5)) == 1200
    assert np.allclose(a[[300, 680, 800, 900]].ravel(), [29.29, 3.426e6, 1191.9, 160.6], rtol=1e-3)
    s = np.load(os.path.join(golden_dir, "cv_small_exact.npz"))
    for key in ("omega", "reference", "dense", "reference_rel_dev"):
        assert s[key].shape == (5,), key
    assert np.all(s["dense"] > 0) and float(s["eta"]) > 0 and int(s["m_max"]) >= 8
    assert np.allclose(np.abs(s["reference"] - s["dense"]) / s["dense"], s["reference_rel_dev"])
