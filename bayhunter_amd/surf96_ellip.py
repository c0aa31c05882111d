"""Rayleigh-wave ellipticity (H/V, the ZH ratio) plugin backed by the MI355X engine.

The reference has no such target -- its users write one as a "user-defined target" (templates/myfwd.py) --, so this class
mirrors `SurfDisp` instead: constructor, `set_modelparams`, `run_model(h, vp, vs, rho, **params) -> (x, y)` with `(nan, nan)` for a
model without a root, and `run_models`, the batched sibling.  The work is bayhunter_amd/csrc/swd_ellip.hip through the C ABI
`bh_swd_ellip` (include/bh_engine_swd_ellip.h): the engine's fundamental-mode Rayleigh phase search, then the ratio of two
components of the compound vector at the polished root.

modelparams
    signed  False (default): y = |hv|, what an amplitude ratio measures; True: hv with its sign (positive = retrograde).
    ratio   "hv" (default) or "zh", the reciprocal.
    nsteps  secant steps of the polish, 0..3 (default 2: hv no longer depends on which search produced the velocity).
"""
import numpy as np

from . import engine as _engine

MAXPERIODS = _engine.MAX_PERIODS


class SurfEllip(object):
    def __init__(self, obsx, ref="rellip", engine=None):
        self.obsx = np.asarray(obsx, dtype=float).reshape(-1)
        self.kmax = self.obsx.size
        if ref != "rellip":
            raise ReferenceError("Reference '%s' is not available in SurfEllip; the available ref is rellip" % ref)
        if not 1 <= self.kmax <= MAXPERIODS:
            # (SurfDisp resamples a longer curve on 60 periods; an H/V curve with a sign change has no such resampling)
            raise ValueError("SurfEllip takes 1..%d periods, not %d" % (MAXPERIODS, self.kmax))
        self.ref = ref
        self.modelparams = {"mode": 1, "flsph": 0, "signed": False, "ratio": "hv", "nsteps": 2}
        self._engine = engine

    @property
    def engine(self):
        if self._engine is None:
            self._engine = _engine.default_engine()
        return self._engine

    def set_modelparams(self, **mparams):
        p = dict(self.modelparams)
        p.update(mparams)
        if p["mode"] != 1:
            raise ValueError("SurfEllip: the fundamental mode only (mode = 1), not mode = %r" % (p["mode"],))
        if p["flsph"] != 0:
            raise ValueError("SurfEllip: flat models only (flsph = 0): earth flattening needs its own correction of the "
                             "eigenfunctions")
        if p["ratio"] not in ("hv", "zh"):
            raise ValueError("SurfEllip: ratio must be 'hv' or 'zh', not %r" % (p["ratio"],))
        if p["nsteps"] not in range(_engine.ELLIP_MAXSTEPS + 1):
            raise ValueError("SurfEllip: nsteps must be 0..%d, not %r" % (_engine.ELLIP_MAXSTEPS, p["nsteps"]))
        self.modelparams = p

    def run_models(self, nlay, h, vp, vs, rho, layout="layer_major"):
        """Batch of models -> (x[K], y[B, K], err[B]).  A model fails in band (err != 0, its row NaN) when the dispersion search
        found no root, when the polish, a value or the gate on the mismatch raised the call's flag (include/bh_engine_swd_ellip.h),
        or when a value is not finite."""
        p = self.modelparams
        out = self.engine.swd_ellip(nlay, h, vp, vs, rho, self.obsx, nsteps=p["nsteps"], layout=layout)
        y = out["hv"]
        if p["ratio"] == "zh":
            with np.errstate(divide="ignore"):
                y = 1.0 / y
        if not p["signed"]:
            y = np.abs(y)
        err = ((out["err"] != 0) | (out["flag"] != 0) | ~np.isfinite(y).all(axis=1)).astype(np.int32)
        y[err != 0] = np.nan
        return self.obsx, y, err

    def run_model(self, h, vp, vs, rho, **params):
        h, vp, vs, rho = [np.asarray(a, dtype=float).reshape(-1, 1) for a in (h, vp, vs, rho)]
        nlay = np.array([h.shape[0]], dtype=np.int32)
        x, y, err = self.run_models(nlay, h, vp, vs, rho)
        if err[0] != 0:
            return np.nan, np.nan
        return x, y[0]
