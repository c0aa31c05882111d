"""The Rayleigh ellipticity target (include/bh_engine_swd_ellip.h, bayhunter_amd/surf96_ellip.py, Targets.RayleighEllipticity), the
parts that need no GPU: the header and the library's export, what the plugin refuses before anything touches the GPU, how the
target describes itself to the engine, and who refuses it."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.sites import SiteTargets
from bayhunter_amd.surf96_ellip import SurfEllip

X = np.array([2.0, 4.0, 8.0, 12.0, 20.0])


def ell_target(x=X, law="nocorr"):
    t = bh.RayleighEllipticity(x, 0.8 + 0.0 * x)
    t.set_noise_law(law)
    return t


def test_library_exports_the_ellipticity_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_swd_ellip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_swd_ellip"]
    assert sorted(E.SWD_ELLIP_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.POSTERIOR_SYMBOLS, E.CHAIN_DIAG_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in ("bh_engine.h", "bh_engine_debug.h"):   # declared in the new header only; the ABI version stays
        assert "bh_swd_ellip" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
    assert lib.bh_abi_version() == 10
    assert b"swd_ellip_kernel" in open(E.LIB_PATH, "rb").read()


def test_plugin_refuses_what_it_cannot_compute_before_the_gpu():
    with pytest.raises(ValueError, match="1..60 periods, not 61"):
        SurfEllip(np.linspace(1, 40, 61))
    with pytest.raises(ValueError, match="1..60 periods, not 61"):
        bh.RayleighEllipticity(np.linspace(1, 40, 61), np.ones(61))
    with pytest.raises(ReferenceError):
        SurfEllip(X, "rdispph")
    p = SurfEllip(X)
    assert p._engine is None
    with pytest.raises(ValueError, match="mode = 1"):
        p.set_modelparams(mode=2)
    with pytest.raises(ValueError, match="flsph = 0"):
        p.set_modelparams(flsph=1)
    with pytest.raises(ValueError, match="ratio"):
        p.set_modelparams(ratio="vh")
    with pytest.raises(ValueError, match="nsteps"):
        p.set_modelparams(nsteps=4)
    assert p.modelparams == {"mode": 1, "flsph": 0, "signed": False, "ratio": "hv", "nsteps": 2}   # a refused update changes nothing
    p.set_modelparams(signed=True, ratio="zh", nsteps=0, mode=1, flsph=0)
    assert (p.modelparams["signed"], p.modelparams["ratio"], p.modelparams["nsteps"]) == (True, "zh", 0)
    assert p._engine is None


def test_target_is_a_user_target_for_the_engine():
    t = ell_target()
    assert (t.ref, t.noiseref) == ("rellip", "ell")
    assert isinstance(t.moddata.plugin, SurfEllip) and not isinstance(t.moddata.plugin, bh.SurfDisp)
    assert t.moddata.xlabel == "Period in s"
    assert not t.engine_backed()
    d = t.engine_desc()
    assert d["kind"] == E.TARGET_USER and d["n"] == X.size and d["law"] == E.LAW_NOCORR
    assert "x" not in d and "iwave" not in d
    assert bh.RayleighDispersionPhase(X, 3.0 + 0 * X).engine_backed()


def test_device_chains_refuse_the_target_by_name():
    import bayhunter_amd.engine as eng_mod
    before = dict(eng_mod._default)
    for targets in ([bh.RayleighDispersionPhase(X, 3.0 + 0 * X), ell_target()],
                    bh.JointTarget([ell_target()])):
        with pytest.raises(E.EngineError, match="RayleighEllipticity"):
            bh.DeviceChains(targets, nchains=4, initparams={"iter_burnin": 8, "iter_main": 8},
                            modelpriors={"ellnoise_corr": 0.0, "ellnoise_sigma": (0.01, 0.2)})
    assert eng_mod._default == before   # no engine was created on the way


def test_site_targets_refuse_the_target():
    sites = [bh.JointTarget([ell_target()]), bh.JointTarget([ell_target()])]
    with pytest.raises(ValueError, match="a user plugin"):
        SiteTargets(sites).check()
