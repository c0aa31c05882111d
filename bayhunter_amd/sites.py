"""Many stations at once: a SITE is one station's observed data for a fixed target structure.

Stations of one array (or nodes of a tomography grid) usually share the periods of their dispersion curves, their
receiver-function parameters and their noise laws; they differ only in the observed values y (and sometimes in yerr).
The forward models depend on the model and x only, so one evaluation batch may mix models of many sites, each compared
with the observed data of its own site (include/bh_engine_sites.h).  `SiteTargets` holds one `JointTarget` per site and
registers site 0's target descriptors plus the table of every site's observed data on the engine.  The ray parameter p and
near-surface velocity nsv of the receiver functions may differ between sites as well (per_site_rf=True,
include/bh_engine_sites_rf.h): they enter only the coefficient stage of the forward model.  So may the periods of the
dispersion curves and their number (per_site_x=True, include/bh_engine_sites_x.h): every model is then searched at the
periods of its own site, as a one-site run searches it.  per_site_x="all" extends that from fundamental-mode phase
velocities to every dispersion target -- group velocities and higher modes (include/bh_engine_sites_x_all.h).  And a station need
not have every target of the array (missing=True, include/bh_engine_sites_missing.h): the targets become SLOTS, a site gives None
in the slots it lacks, and each of its models is evaluated -- and each of its chains walks -- as in a one-site run over the targets
the site has.  The fixed noise correlation of a Gauss-law target -- a receiver function's usual configuration -- may differ between
sites too (per_site_corr=True, include/bh_engine_sites_gauss.h): the sites' matrices R^-1 are registered once per distinct value.
And so may a receiver function's time axis and Gauss filter (per_site_rf="all", include/bh_engine_sites_rf_axis.h): window, sampling
rate, sample count and filter width are then a station's own, and each model's trace is synthesised on its site's axis.
Last, the installed noise LAW of a slot may differ between sites (per_site_law=True, include/bh_engine_sites_laws.h): the sampler
installs a target's law from the station's own priors and data, so stations with their own priors differ in them.
The Rayleigh ellipticity (H/V) slot follows the dispersion slots in all of this with per_site_ellip=True
(include/bh_engine_sites_ellip.h): its periods and their number are then a station's own, and a station may lack it.
"""
import numpy as np

from . import engine as _engine
from .Targets import JointTarget, LAWS
from .rfmini_modrf import RFminiModRF
from .surf96_modsw import SurfDisp
from .surf96_ellip import SurfEllip

# the most periods a site may have with per_site_x=True (beyond them a one-site run interpolates: surf96_modsw.py)
SITE_X_MAX_PERIODS = 60


def window_site_map(nchains, nsites, ld):
    """Site of every column of a speculative window (include/bh_engine.h: node j of chain c in column j*C + c, with
    C = nsites * nchains chains, site s holding chains s*nchains .. (s+1)*nchains - 1): int32 [ld]."""
    C = int(nsites) * int(nchains)
    return ((np.arange(int(ld), dtype=np.int64) % C) // int(nchains)).astype(np.int32)


# what the noise entries of a slot a site lacks hold in the slot layout (never proposed, never checked, never read)
ABSENT_NOISE = 0.0


def slot_columns(present):
    """The columns of a site's OWN layout inside the slot layout, from its row `present[nslots]` of booleans: (noise columns --
    two per present slot, in order --, misfit columns -- one per present slot, then the joint misfit's)."""
    present = np.asarray(present, dtype=bool)
    idx = np.flatnonzero(present)
    return np.column_stack((2 * idx, 2 * idx + 1)).ravel(), np.concatenate((idx, [present.size]))


def scatter_slots(present, noise, misfits):
    """A site's own noise[..., 2k] and misfits[..., k + 1] (k = the targets it has) in the slot layout: (noise[..., 2 nslots] with
    ABSENT_NOISE in the slots it lacks, misfits[..., nslots + 1] with 0 there); the joint misfit stays last."""
    ncol, mcol = slot_columns(present)
    noise, misfits = np.asarray(noise, dtype=float), np.asarray(misfits, dtype=float)
    nslots = np.asarray(present).size
    on = np.full(noise.shape[:-1] + (2 * nslots,), ABSENT_NOISE)
    om = np.zeros(misfits.shape[:-1] + (nslots + 1,))
    on[..., ncol], om[..., mcol] = noise, misfits
    return on, om


def gather_slots(present, noise, misfits):
    """The inverse of scatter_slots: the site's own columns of noise[..., 2 nslots] and misfits[..., nslots + 1]."""
    ncol, mcol = slot_columns(present)
    return np.asarray(noise)[..., ncol], np.asarray(misfits)[..., mcol]


def _law_or_none(t):
    """t.law(), or None while no law is installed (the sampler installs it)"""
    try:
        return t.law()
    except RuntimeError:
        return None


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


# the parameters of an ellipticity plugin the sites of a slot must agree in (the engine registers one forward model per slot)
SITE_ELLIP_PARAMS = ("nsteps", "signed", "ratio")
# the receiver-function call arguments that may differ between sites with per_site_rf=True (RFminiModRF._call_args)
SITE_RF_ARGS = ("p", "nsv")
# ... and with per_site_rf="all": everything but the wave type
SITE_RF_AXIS_ARGS = SITE_RF_ARGS + ("gauss", "nsamp", "fsamp", "tshift", "nkeep")
# the longest transform of a site with per_site_rf="all" (include/bh_engine_sites_rf_axis.h: BH_SITES_RF_AXIS_MAX_NSAMP)
SITE_RF_AXIS_MAX_NSAMP = 16384


class SiteTargets(object):
    """One `JointTarget` per site, evaluated together.  Every site must have the same number and classes of targets, the
    same x (bit for bit), the same plugin parameters (SWD mode / flsph, every receiver-function call argument), the same
    installed noise law and -- Gauss law -- identical corr_inv and logcorr_det; only engine-backed plugins.  y and yerr
    may differ.  The checks run when the sites are registered (the noise laws are installed by the sampler).

    per_site_rf=True: the receiver-function plugins of the sites may also differ in their ray parameter `p` and near-surface
    velocity `nsv` (a station's slowness depends on the events it recorded); every other receiver-function argument (gauss,
    nsamp, fsamp, tshift, wave type, nkeep) must still match.  Each model is then computed with its own site's p and nsv.
    The default (False) rejects a differing p or nsv like any other mismatch.

    per_site_x=True: the dispersion targets of fundamental-mode phase velocity may also differ in their periods x and in the
    number of them (1 to 60 per site; not with the Gauss law, whose R^-1 depends on the number).  Each model's curve is then
    computed at its own site's periods and compared over its own site's samples; in the synthetics a site's velocities are
    followed by zeros up to the largest count of any site.  Group-velocity and higher-mode targets and receiver functions
    still share x bit for bit.  The default (False) keeps the check above.

    per_site_x="all": as True, for EVERY dispersion target -- phase or group velocity, modes 1 to 3, Rayleigh or Love, flat or
    flattened: group-velocity and higher-mode targets may differ in their periods and their number as well (a station's group
    curve has its own usable band just as its phase curve has).  A group velocity's two roots per period and the mode loop
    are searched at the model's own site's periods -- the bits of a one-site run.  Receiver functions still share x.

    per_site_rf="all" (needs per_site_x="all"): as True, and the receiver functions of the sites may differ in their time axis x as
    well -- hence in nsamp, fsamp, tshift and the number of samples -- and in the filter width `gauss`; only the wave type and the
    noise law must match.  Each model's trace is then synthesised on its own site's axis with its own site's filter, the bits of a
    one-site run over the site's samples; in the synthetics a site's samples are followed by zeros up to the largest count of any
    site.  A site's transform has at most 16384 points (8192 observed samples).  Under the Gauss law the shapes of corr_inv follow
    the sample counts; sites whose counts differ then need per_site_corr=True (`gauss_class_arrays` embeds every site's matrix
    in a zero matrix of the capacity).

    missing=True (needs per_site_x="all"): a site may LACK some of the array's targets.  Every site is then a sequence of the
    same length, target or None: position i is SLOT i, which has one class, one plugin parameter set and one noise law wherever
    it is present (the checks above, among the sites that have it); every slot is present at one site or more and every site has
    one target or more.  `ntargets` and `targets` describe the slots (a slot's descriptor is that of the first site that has
    it), noise and misfits of `evaluate_batch` are in the slot layout; `site(s)` is the JointTarget of the targets site s HAS --
    the one-site run its models and chains reproduce.  For a slot the model's site lacks nothing is added to logL or the joint
    misfit, its misfit is 0, it never sets err, its synthetics are zeros and its forward model is not run.  Refused without per_site_corr:
    the Gauss law on a slot that some site lacks.

    per_site_corr=True: the sites' Gauss-law targets may differ in corr_inv / logcorr_det -- every station fixes its own noise
    correlation -- provided the shapes are equal (the sample count stays shared).  The sites' matrices are deduplicated by their
    bits into correlation CLASSES and one table per Gauss-law target is registered (`gauss_class_arrays`,
    Engine.set_sites_gauss); each model is contracted with its own site's matrix, the bits of its one-site evaluation in a
    batch of the same size.  With missing=True a Gauss-law slot may then be absent at some sites (class -1).  Still refused: a
    Gauss-law dispersion target with periods per site; without per_site_law, sites whose installed laws differ ('gauss' against
    'exp').

    per_site_law=True (needs missing=True): the sites' installed noise laws may differ slot by slot -- error bars at one station
    and none at another ('nocorr_scalederr' / 'nocorr'), a correlation ranged at one and fixed at its neighbour ('exp' /
    'gauss').  One table of laws (`site_law_arrays`, Engine.set_sites_laws) is registered after the count and
    receiver-function tables and before the correlation classes; each model is evaluated under its own site's laws, the bits of
    an evaluation of the same batch in which every site has them.  A slot's descriptor is then that of the first site that has
    it under the Gauss law, if any (the descriptor owns the contraction's shape), else of the first site that has it; Gauss
    matrices are compared among the Gauss sites only, and the sites under another law are in class -1 of `gauss_class_arrays`.
    The flag SWITCHES per_site_corr ON: a Gauss-law slot with a site under another law needs the class table in any case, and
    stations that differ in their laws fix their correlations independently.  Still refused: the Gauss law on a dispersion
    target (periods per site).

    A `RayleighEllipticity(fused=True)` slot (include/bh_engine_ellip_target.h) is engine-backed and admitted: its periods x and
    its plugin's nsteps / signed / ratio are shared by all sites, whatever per_site_x gives the DISPERSION slots beside it
    (under a table of periods per site the ellipticity runs a phase-velocity search of its own at its shared periods).  Without
    per_site_ellip not with missing=True (hence not with per_site_law): every site then has the ellipticity.

    per_site_ellip=True (needs per_site_x="all"; include/bh_engine_sites_ellip.h): the ellipticity slot's periods x and their number
    (1 to 60 per site; not with the Gauss law) may differ between sites as a dispersion slot's do -- a station's H/V curve has its
    own usable band, rarely its phase-velocity curve's; nsteps / signed / ratio stay shared.  With missing=True the slot may then be
    None at a site, and per_site_law=True is open to it.  Each model's ellipticities are computed at its own site's periods, the
    bits of a one-site run; in the synthetics they are followed by zeros up to the largest count of any site.  Where, at every
    site that has the ellipticity, the site's Rayleigh phase-velocity slot has the same periods bit for bit, the ellipticity
    reads that slot's velocities and costs no search of its own.  Without the flag every check above is what it was."""

    def __init__(self, jointtargets, names=None, engine=None, per_site_rf=False, per_site_x=False, missing=False, per_site_corr=False,
                 per_site_law=False, per_site_ellip=False):
        self.per_site_ellip = bool(per_site_ellip)
        if self.per_site_ellip and per_site_x != "all":
            raise ValueError("per_site_ellip=True needs per_site_x=\"all\" (the table of counts it extends)")
        self.missing = bool(missing)
        self.per_site_law = bool(per_site_law)
        if self.per_site_law and not self.missing:
            raise ValueError("per_site_law=True needs missing=True (the table of counts it extends)")
        self.per_site_corr = bool(per_site_corr) or self.per_site_law
        self._slots = None
        if self.missing:
            if per_site_x != "all":
                raise ValueError("missing=True needs per_site_x=\"all\" (the table of counts it extends)")
            jointtargets = self._take_slots(jointtargets)
        self._sites = [jt if isinstance(jt, JointTarget) else JointTarget(jt) for jt in jointtargets]
        if not self._sites:
            raise ValueError("SiteTargets needs at least one site")
        self._names = ["site%03d" % s for s in range(len(self._sites))] if names is None else [str(n) for n in names]
        if len(self._names) != len(self._sites) or len(set(self._names)) != len(self._names):
            raise ValueError("names must be %d distinct names, one per site" % len(self._sites))
        self._engine = engine
        if isinstance(per_site_rf, str) and per_site_rf != "all":
            raise ValueError("per_site_rf is False, True or \"all\", not %r" % (per_site_rf,))
        self.per_site_rf = "all" if isinstance(per_site_rf, str) else bool(per_site_rf)
        if self.per_site_rf == "all" and per_site_x != "all":
            raise ValueError("per_site_rf=\"all\" needs per_site_x=\"all\" (the table of counts it extends)")
        if isinstance(per_site_x, str) and per_site_x != "all":
            raise ValueError("per_site_x is False, True or \"all\", not %r" % (per_site_x,))
        self.per_site_x = "all" if isinstance(per_site_x, str) else bool(per_site_x)
        for jt in self._sites:          # every site on one engine
            if jt._engine is None:
                jt._engine = engine
        self._registered = None

    def _take_slots(self, sites):
        """missing=True: the sites as rows of slots (self._slots[s][i]: target or None), checked for shape; returns every site's
        present targets"""
        slots = [list(jt.targets) if isinstance(jt, JointTarget) else list(jt) for jt in sites]
        if not slots:
            raise ValueError("SiteTargets needs at least one site")
        nslots = len(slots[0])
        for s, row in enumerate(slots):
            if len(row) != nslots:
                raise ValueError("site %d gives %d slots, site 0 gives %d (None marks a target the site lacks)" % (s, len(row), nslots))
            if all(t is None for t in row):
                raise ValueError("site %d has no target (every slot None)" % s)
        for i in range(nslots):
            if all(row[i] is None for row in slots):
                raise ValueError("slot %d is present at no site" % i)
        self._slots = slots
        return [[t for t in row if t is not None] for row in slots]

    @property
    def present(self):
        """bool [nsites, ntargets]: site s has the target of slot i (all True without missing=True)"""
        if self._slots is None:
            return np.ones((self.nsites, self.ntargets), dtype=bool)
        return np.array([[t is not None for t in row] for row in self._slots], dtype=bool)

    def _slot_rows(self):
        """every site's targets by slot (None: the site lacks it)"""
        return self._slots if self._slots is not None else [jt.targets for jt in self._sites]

    # ---- the JointTarget surface the chain drivers use -----------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            self._engine = self._sites[0].engine
        for jt in self._sites:          # every site on the same engine
            if jt._engine is None:
                jt._engine = self._engine
        return self._engine

    @property
    def targets(self):
        """site 0's targets (the target structure every site shares); missing=True: every slot's target at the first site that
        has it"""
        if self._slots is not None:
            return [self._slots[self._slot_site(i)][i] for i in range(len(self._slots[0]))]
        return self._sites[0].targets

    def _slot_site(self, i):
        """the site whose target describes slot i: the first that has it; per_site_law=True: the first that has it under the
        Gauss law, if any (the descriptor owns the contraction's shape and workspace)"""
        have = [s for s, row in enumerate(self._slots) if row[i] is not None]
        if self.per_site_law:
            for s in have:
                if _law_or_none(self._slots[s][i]) == "gauss":
                    return s
        return have[0]

    @property
    def ntargets(self):
        return len(self._slots[0]) if self._slots is not None else self._sites[0].ntargets

    @property
    def nsites(self):
        return len(self._sites)

    @property
    def names(self):
        return list(self._names)

    def site(self, s):
        """the JointTarget of site s (missing=True: of the targets it has -- the one-site run)"""
        return self._sites[int(s)]

    # ---- checks and registration -------------------------------------------------------------------
    def check(self):
        """Raise ValueError unless every site shares site 0's target structure (class docstring); missing=True: unless every
        slot is one target structure among the sites that have it."""
        if self._slots is not None:
            return self._check_slots()
        ref = self._sites[0]
        for s, jt in enumerate(self._sites):
            who = "site %d (%s)" % (s, self._names[s])
            if jt.ntargets != ref.ntargets:
                raise ValueError("%s has %d targets, site 0 has %d" % (who, jt.ntargets, ref.ntargets))
            for i, (t, t0) in enumerate(zip(jt.targets, ref.targets)):
                self._check_target("%s, target %d (%s)" % (who, i, t.ref), t, t0, "site 0")

    def _check_slots(self):
        """missing=True: the checks of `check` slot by slot, every site that has the slot against the first one that has it"""
        for i in range(self.ntargets):
            have = [s for s, row in enumerate(self._slots) if row[i] is not None]
            first = self._slot_site(i)
            t0 = self._slots[first][i]
            if isinstance(t0.moddata.plugin, SurfEllip) and not self.per_site_ellip:
                raise ValueError("site %d (%s), slot %d (%s): missing=True does not serve a %s slot (every site has the ellipticity, "
                                 "at shared periods)" % (first, self._names[first], i, getattr(t0, "ref", "?"), type(t0).__name__))
            for s in have:
                t = self._slots[s][i]
                what = "site %d (%s), slot %d (%s)" % (s, self._names[s], i, getattr(t, "ref", "?"))
                self._check_target(what, t, t0, "site %d" % first)
                if len(have) < self.nsites and t.law() == "gauss" and not self.per_site_corr:
                    raise ValueError("%s: Gauss law on a slot that some site lacks (the contraction gathers every site's rows)" % what)

    def _check_target(self, what, t, t0, whose):
        """target t (`what`, for the messages) against the target t0 of site `whose` it must share its structure with"""
        if not t.engine_backed():
            raise ValueError("%s: a user plugin; a site set takes engine-backed targets only" % what)
        if type(t) is not type(t0):
            raise ValueError("%s is a %s, %s's is a %s" % (what, type(t).__name__, whose, type(t0).__name__))
        x, x0 = np.asarray(t.obsdata.x, dtype=float), np.asarray(t0.obsdata.x, dtype=float)
        same_x = x.shape == x0.shape and _bits(x) == _bits(x0)
        site_x = self.per_site_x and isinstance(t.moddata.plugin, SurfDisp) and isinstance(t0.moddata.plugin, SurfDisp)
        site_axis = (self.per_site_rf == "all" and isinstance(t.moddata.plugin, RFminiModRF)
                     and isinstance(t0.moddata.plugin, RFminiModRF))
        site_ellip = self.per_site_ellip and isinstance(t.moddata.plugin, SurfEllip) and isinstance(t0.moddata.plugin, SurfEllip)
        if not same_x and not site_x and not site_axis and not site_ellip:
            raise ValueError("%s: x differs from %s's (sites share x bit for bit)" % (what, whose))
        if site_x:
            self._check_site_x(what, t, x, same_x)
        if site_ellip:
            self._check_site_ellip(what, t, x)
        if site_axis and t.moddata.plugin.nsamp > SITE_RF_AXIS_MAX_NSAMP:
            raise ValueError("%s: %d samples need a transform of %d points; a site has at most %d with per_site_rf=\"all\""
                             % (what, x.size, t.moddata.plugin.nsamp, SITE_RF_AXIS_MAX_NSAMP))
        if np.size(t.obsdata.y) != x.size:
            raise ValueError("%s: y has %d values for %d samples" % (what, np.size(t.obsdata.y), x.size))
        p, p0 = t.moddata.plugin, t0.moddata.plugin
        if type(p) is not type(p0):
            raise ValueError("%s: plugin %s, %s's is %s" % (what, type(p).__name__, whose, type(p0).__name__))
        if isinstance(p, SurfDisp):
            a = (p.wavetype, p.veltype, p.modelparams["mode"], p.modelparams["flsph"])
            a0 = (p0.wavetype, p0.veltype, p0.modelparams["mode"], p0.modelparams["flsph"])
            if a != a0:
                raise ValueError("%s: dispersion parameters (wave, velocity, mode, flsph) %r, %s's %r" % (what, a, whose, a0))
        elif isinstance(p, SurfEllip):
            a, a0 = [tuple(q.modelparams[k] for k in SITE_ELLIP_PARAMS) for q in (p, p0)]
            if a != a0:
                raise ValueError("%s: ellipticity parameters (nsteps, signed, ratio) %r, %s's %r" % (what, a, whose, a0))
        elif isinstance(p, RFminiModRF):
            a, a0 = p._call_args(), p0._call_args()
            if self.per_site_rf:
                free = SITE_RF_AXIS_ARGS if self.per_site_rf == "all" else SITE_RF_ARGS
                a, a0 = [{k: v for k, v in d.items() if k not in free} for d in (a, a0)]
            if a != a0:
                raise ValueError("%s: receiver-function parameters %r, %s's %r" % (what, a, whose, a0))
        law, law0 = t.law(), t0.law()
        if law != law0 and not self.per_site_law:
            raise ValueError("%s: noise law %r, %s's %r" % (what, law, whose, law0))
        if law == "gauss" and law0 == "gauss":   # (per_site_law: t0 is the slot's first Gauss site -- among the Gauss sites only)
            v, v0 = t.valuation, t0.valuation
            if self.per_site_corr:
                if np.shape(v.corr_inv) != np.shape(v0.corr_inv) and not site_axis:
                    raise ValueError("%s: Gauss law with R^-1 of shape %r, %s's %r (sites share the sample count)"
                                     % (what, np.shape(v.corr_inv), whose, np.shape(v0.corr_inv)))
            elif (np.shape(v.corr_inv) != np.shape(v0.corr_inv) or _bits(v.corr_inv) != _bits(v0.corr_inv)
                    or _bits(v.logcorr_det) != _bits(v0.logcorr_det)):
                raise ValueError("%s: Gauss law with another R^-1 / ln|R| than %s's (sites share corr)" % (what, whose))

    def _check_site_x(self, what, t, x, same_x):
        """what the engine refuses of a dispersion target registered with periods per site (include/bh_engine_sites_x.h; with
        per_site_x="all" include/bh_engine_sites_x_all.h, which serves group velocities and higher modes too);
        same_x: the site's x is site 0's"""
        p = t.moddata.plugin
        if self.per_site_x != "all" and not same_x and (p.veltype != 0 or p.modelparams["mode"] > 1):
            raise ValueError("%s: x differs from site 0's on a group-velocity or higher-mode target (per_site_x serves "
                             "fundamental-mode phase velocities)" % what)
        if x.ndim != 1 or x.size < 1 or x.size > SITE_X_MAX_PERIODS:
            raise ValueError("%s: %d periods; a site has 1 to %d with per_site_x" % (what, x.size, SITE_X_MAX_PERIODS))
        if not np.all(np.isfinite(x) & (x > 0)):
            raise ValueError("%s: a period that is not finite and positive" % what)
        if t.law() == "gauss":
            raise ValueError("%s: Gauss law on a dispersion target with periods per site (R^-1 depends on their number)" % what)

    def _check_site_ellip(self, what, t, x):
        """what the engine refuses of an ellipticity target registered with periods per site (include/bh_engine_sites_ellip.h): the
        rules of a dispersion target"""
        if x.ndim != 1 or x.size < 1 or x.size > SITE_X_MAX_PERIODS:
            raise ValueError("%s: %d periods; a site has 1 to %d with per_site_ellip" % (what, x.size, SITE_X_MAX_PERIODS))
        if not np.all(np.isfinite(x) & (x > 0)):
            raise ValueError("%s: a period that is not finite and positive" % what)
        if t.law() == "gauss":
            raise ValueError("%s: Gauss law on an ellipticity target with periods per site (R^-1 depends on their number)" % what)

    def site_x_arrays(self):
        """(n[S, nt] int32, x[S, ldy], yobs[S, ldy], yerr[S, ldy] or None) for Engine.set_sites_x: the samples of every (site,
        target) and every site's x, observed data and errors in ymod's column layout, where a target's columns are as many as
        its largest count over the sites; beyond a site's own count x and yobs hold 0 and yerr 1 (unread).  missing=True
        (Engine.set_sites_missing): count 0 and those placeholders throughout for a slot the site lacks."""
        S, nt = self.nsites, self.ntargets
        n = self._counts()
        cap = n.max(axis=0)
        off = np.concatenate([[0], np.cumsum(cap)]).astype(int)
        scaled = any(LAWS[t.law()] == LAWS["nocorr_scalederr"] for t in self.targets)
        if self.per_site_law:   # (yerr exactly in the (site, slot) cells under that law, by the site's own law)
            scaled = bool((self.site_law_arrays() == LAWS["nocorr_scalederr"]).any())
        x, yobs = np.zeros((S, off[-1])), np.zeros((S, off[-1]))
        yerr = np.ones((S, off[-1])) if scaled else None
        for s, row in enumerate(self._slot_rows()):
            for i, t in enumerate(row):
                if t is None:
                    continue
                c = slice(off[i], off[i] + n[s, i])
                x[s, c] = np.asarray(t.obsdata.x, dtype=float).ravel()
                yobs[s, c] = np.asarray(t.obsdata.y, dtype=float).ravel()
                if scaled and LAWS[t.law()] == LAWS["nocorr_scalederr"]:
                    yerr[s, c] = np.asarray(t.obsdata.yerr, dtype=float).ravel()
        return n, x, yobs, yerr

    def site_law_arrays(self):
        """int32 [nsites, ntargets]: the installed noise law of every (site, slot) (Engine.set_sites_laws); where the site lacks the
        slot the slot descriptor's law, which is not read"""
        desc = [LAWS[t.law()] for t in self.targets]
        return np.array([[desc[i] if t is None else LAWS[t.law()] for i, t in enumerate(row)] for row in self._slot_rows()],
                        dtype=np.int32).reshape(self.nsites, self.ntargets)

    def _counts(self):
        """int32 [nsites, ntargets]: the samples of every (site, target); 0 where the site lacks the slot"""
        return np.array([[0 if t is None else np.size(t.obsdata.x) for t in row] for row in self._slot_rows()],
                        dtype=np.int32).reshape(self.nsites, self.ntargets)

    def _capacity_descs(self):
        """site 0's descriptors; a fundamental-mode phase-velocity target's n is the largest count of any site and its x, yobs
        (and yerr) placeholders of that length -- the site path reads the tables, never these.  Group-velocity and higher-mode
        targets keep site 0's x, which every site shares: the engine checks the table against it, and a group velocity's
        second roots are searched at the descriptor's periods.  per_site_x="all": every dispersion target gets the capacity
        and placeholders -- all of them are searched at the table's periods."""
        n = self._counts()
        descs = []
        for i, t in enumerate(self.targets):
            d = t.engine_desc()
            if d["kind"] == _engine.TARGET_RF and self.per_site_rf == "all":
                # (a receiver function's columns hold the largest count too; nsamp is the largest transform of any site, the other
                # axis values and the Gauss law's matrix are placeholders: the site path reads the tables)
                cap = int(n[:, i].max())
                d["n"] = cap
                d["yobs"] = np.zeros(cap)
                d["nsamp"] = max(int(row[i].moddata.plugin.nsamp) for row in self._slot_rows() if row[i] is not None)
                if "yerr" in d:
                    d["yerr"] = np.ones(cap)
                if "rinv" in d and self.per_site_corr:   # (without it every site shares the descriptor's matrix, of one size)
                    d["rinv"], d["logdet_r"] = np.eye(cap), 0.0
            if d["kind"] == _engine.TARGET_SWD and (self.per_site_x == "all" or (d["igr"] == 0 and d["mode"] <= 1)):
                cap = int(n[:, i].max())
                d["n"] = cap
                d["x"], d["yobs"] = np.ones(cap), np.zeros(cap)
                if "yerr" in d:
                    d["yerr"] = np.ones(cap)
            if self.per_site_ellip and d["kind"] == _engine.TARGET_USER and "nsteps" in d:
                # (the ellipticity slot likewise; Engine.set_targets makes the key the call of bh_targets_set_ellip_sites)
                cap = int(n[:, i].max())
                d["n"] = cap
                d["x"], d["yobs"] = np.ones(cap), np.zeros(cap)
                if "yerr" in d:
                    d["yerr"] = np.ones(cap)
                d["ellip_sites"] = True
            descs.append(d)
        return descs

    def site_arrays(self):
        """(yobs[S, ldy], yerr[S, ldy] or None): every site's observed data, target after target as in ymod"""
        yobs = np.vstack([np.concatenate([np.asarray(t.obsdata.y, dtype=float).ravel() for t in jt.targets])
                          for jt in self._sites])
        if not any(LAWS[t.law()] == LAWS["nocorr_scalederr"] for t in self.targets):
            return yobs, None
        yerr = np.vstack([np.concatenate([np.asarray(t.obsdata.yerr, dtype=float).ravel() for t in jt.targets])
                          for jt in self._sites])
        return yobs, yerr

    def site_rf_arrays(self):
        """(p[S, nt], nsv[S, nt]): every site's receiver-function ray parameter (s/deg) and near-surface velocity (0: the
        model's top-layer vs) in the columns of its receiver-function targets, 0 elsewhere (Engine.set_sites_rf)"""
        S, nt = self.nsites, self.ntargets
        p, nsv = np.zeros((S, nt)), np.zeros((S, nt))
        for s, row in enumerate(self._slot_rows()):
            for i, t in enumerate(row):
                if t is not None and isinstance(t.moddata.plugin, RFminiModRF):
                    a = t.moddata.plugin._call_args()
                    p[s, i], nsv[s, i] = float(a["p"]), float(a["nsv"])
        return p, nsv

    def site_rf_axis_arrays(self):
        """(nsamp[S, nt] int32, fsamp[S, nt], tshift[S, nt], gauss[S, nt]): every site's receiver-function transform length,
        sampling rate (Hz), time shift (s) and Gauss width in the columns of its receiver-function targets; placeholders (4, 1, 0,
        1: never read) elsewhere and where the site lacks the slot (Engine.set_sites_rf_axis)"""
        S, nt = self.nsites, self.ntargets
        nsamp = np.full((S, nt), 4, dtype=np.int32)
        fsamp, tshift, gauss = np.ones((S, nt)), np.zeros((S, nt)), np.ones((S, nt))
        for s, row in enumerate(self._slot_rows()):
            for i, t in enumerate(row):
                if t is not None and isinstance(t.moddata.plugin, RFminiModRF):
                    a = t.moddata.plugin._call_args()
                    nsamp[s, i], fsamp[s, i], tshift[s, i], gauss[s, i] = a["nsamp"], a["fsamp"], a["tshift"], a["gauss"]
        return nsamp, fsamp, tshift, gauss

    def gauss_class_arrays(self):
        """per_site_corr=True: {slot: (class_of[S] int32, rinv[nclass, n, n], logdet_r[nclass])} for Engine.set_sites_gauss, one
        entry per Gauss-law slot.  The sites' (corr_inv, logcorr_det) are deduplicated by their bits, classes numbered in the
        order of their first site; -1: the site lacks the slot.  per_site_rf="all": n is the slot's capacity, a site's own matrix
        sits in the top-left corner of a zero matrix of that size (the residuals beyond its samples are exact zeros), and the
        classes are deduplicated by (bits, own size)."""
        out = {}
        caps = self._counts().max(axis=0)
        for i, t0 in enumerate(self.targets):
            if t0.law() != "gauss":
                continue
            seen, class_of, rinv, logdet = {}, [], [], []
            for row in self._slot_rows():
                t = row[i]
                if t is None or t.law() != "gauss":   # (per_site_law: a site under another law belongs to no class either)
                    class_of.append(-1)
                    continue
                v = t.valuation
                own = np.asarray(v.corr_inv, dtype=np.float64)
                key = (_bits(own), _bits(v.logcorr_det), own.shape)
                if key not in seen:
                    seen[key] = len(rinv)
                    if own.shape[0] < caps[i]:
                        own, corner = np.zeros((caps[i], caps[i])), own
                        own[:corner.shape[0], :corner.shape[1]] = corner
                    rinv.append(own)
                    logdet.append(float(v.logcorr_det))
                class_of.append(seen[key])
            out[i] = (np.array(class_of, dtype=np.int32), np.stack(rinv), np.array(logdet, dtype=np.float64))
        return out

    def _signature(self):
        """What the registration depends on, by identity as JointTarget._signature: every site's targets, plugins and laws,
        and the arrays of its x, y and yerr (O(sites x targets) per call; replacing an array re-registers)."""
        return tuple((jt._signature(), tuple((id(t.obsdata.x), id(t.obsdata.y), id(t.obsdata.yerr)) for t in jt.targets))
                     for jt in self._sites)

    def _register(self):
        """Site 0's descriptors + the site table on the engine, checked (`check`) and registered again only when the signature
        changed or another caller registered its own targets since (Engine._owner)."""
        sig = self._signature()
        e = self.engine
        if self._registered != sig:
            self.check()
        if self._registered != sig or e._owner is not self:
            if self.per_site_x:
                e.set_targets(self._capacity_descs())
                tables = self.site_x_arrays()
                if self.per_site_rf == "all":
                    e.set_sites_axes(*tables)
                elif self.missing and self.per_site_corr:
                    e.set_sites_missing_gauss(*tables)
                elif self.missing:
                    e.set_sites_missing(*tables)
                elif self.per_site_x == "all":
                    e.set_sites_x_all(*tables)
                else:
                    e.set_sites_x(*tables)
            else:
                e.set_targets([t.engine_desc() for t in self.targets])
                yobs, yerr = self.site_arrays()
                e.set_sites(yobs, yerr)
            if self.per_site_rf or self.missing:   # (missing: the coefficient stage finds the model's site through this table)
                e.set_sites_rf(*self.site_rf_arrays())
            if self.per_site_rf == "all":
                e.set_sites_rf_axis(*self.site_rf_axis_arrays())
            if self.per_site_law:                  # (after the count and receiver-function tables, before the classes it drops)
                e.set_sites_laws(self.site_law_arrays(), tables[3])   # (the errors of the count-table call)
            if self.per_site_corr:                 # (last: every other registration drops the classes)
                for i, (class_of, rinv, logdet) in sorted(self.gauss_class_arrays().items()):
                    e.set_sites_gauss(i, class_of, rinv, logdet)
            e._owner = self
            self._registered = sig
            # the arrays the signature names stay alive while it is in force: their ids cannot be handed to replacements
            self._held = [(t.obsdata.x, t.obsdata.y, t.obsdata.yerr) for jt in self._sites for t in jt.targets]

    def evaluate_batch(self, nlay, h, vp, vs, noise, site, rho=None, layout="layer_major", want_ymod=False):
        """B models, model b compared with site site[b]: returns (logL[B], misfits[B, nt+1], err[B][, ymod]).  missing=True:
        noise and misfits in the slot layout (`scatter_slots`)."""
        self._register()
        return self.engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, layout=layout, want_ymod=want_ymod)
