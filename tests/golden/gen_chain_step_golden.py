"""Record single steps of the reference's chain (src/SingleChain.py) for tests/test_chain_ref.py -> chain_step_golden.npz.

Needs the reference (gen_golden.import_reference; `make -C oracle ref` first).  One SingleChain is built as gen_golden.py does
for its recorded runs; its RandomState is swapped for philox_ref.InjectedRandomState, its targets for a stand-in whose
`evaluate` hands back a likelihood chosen by the case, and its own `iterate` is called once per case with the chain's fields set
to the case: state, priors, widths, counters, iteration.  What the reference's own methods return during that call is recorded:
_get_modelproposal and _validmodel, _get_hyperparameter_proposal and _validnoise, _get_vpvs_proposal and _validvpvs, the layered
model handed to evaluate (Models.get_vp_vs_h), get_acceptance_probability, the counters and what adjust_propdist made of the widths,
and the move `iterate` chose (early-phase boundary included).  The cases come from tests/chain_ref.py's crafted lists and random
states; the file holds the cases' inputs and the recorded outputs only.

    python tests/golden/gen_chain_step_golden.py
"""
import os
import sys
import tempfile
from multiprocessing import sharedctypes

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden                                      # noqa: E402
import chain_ref as R                                  # noqa: E402
from philox_ref import InjectedRandomState             # noqa: E402

MLP, NTP = 9, 3                                        # padded widths of the fixture's arrays
SHAPES = ((4, 1), (9, 3))
ITERS = (-1000, -988, -987, 0, 200, 1000)              # early with adaptation, either side of the early-phase boundary, ...
SCALARS = ("layermin", "layermax", "vsmin", "vsmax", "zmin", "zmax", "thickmin", "lvz", "hvz", "vpvsmin", "vpvsmax", "mantle_vs",
           "mantle_vpvs", "acc_lo", "acc_hi", "iter_burnin", "iterations", "iiter", "absent", "ML", "nt", "n", "vpvs", "like", "newlike")


class Recorder(object):
    """the chain's `targets`: evaluate() keeps the layered model it was handed and answers with the case's likelihood"""

    def __init__(self):
        self.seen, self.like, self.misfits = None, 0.0, None

    def evaluate(self, h, vp, vs, noise):
        self.seen = (np.array(h), np.array(vp), np.array(vs), np.array(noise))
        self.proposallikelihood = self.like
        self.proposalmisfits = self.misfits


def make_chain():
    Targets, _, _ = gen_golden.import_reference()
    SingleChain = sys.modules["BayHunter.SingleChain"].SingleChain
    g = np.load(os.path.join(HERE, "chain_golden.npz"))
    jt = Targets.JointTarget(targets=[Targets.RayleighDispersionPhase(g["xsw"], g["ysw"])])
    tmp = tempfile.mkdtemp(prefix="bhstep_")
    priors = dict(vpvs=(1.4, 2.1), layers=(1, 10), vs=(2, 5), z=(0, 60), mohoest=None, swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.05))
    init = dict(nchains=1, iter_burnin=20, iter_main=10, acceptance=(40, 80), thickmin=0.1, lvz=None, hvz=None, rcond=1e-5,
                maxmodels=100, savepath=tmp, station="gold")
    nmodels, maxlayers = int(30 * 80 / 100.), 11
    shared = [sharedctypes.RawArray("f", k) for k in (nmodels * maxlayers * 2, nmodels * 2, nmodels, nmodels * 2, nmodels)]
    return SingleChain(targets=jt, chainidx=0, initparams=init, modelpriors=priors, sharedmodels=shared[0], sharedmisfits=shared[1],
                       sharedlikes=shared[2], sharednoise=shared[3], sharedvpvs=shared[4], random_seed=5)


def install(chain, pr, st, iiter, d6, rec):
    """the chain's fields <- the case (what __init__ and run_chain set, SingleChain.py:27-66, :591-602)"""
    chain.priors = dict(layers=pr["layers"], vs=pr["vs"], z=pr["z"], mantle=pr["mantle"],
                        vpvs=np.float64(pr["vpvs"][0]) if pr["vpvs"][0] == pr["vpvs"][1] else pr["vpvs"])
    chain.dv = pr["vs"][1] - pr["vs"][0]
    chain.thickmin, chain.lowvelperc, chain.highvelperc, chain.mantle = pr["thickmin"], pr["lvz"], pr["hvz"], pr["mantle"]
    chain.acceptance = pr["acceptance"]
    chain.noiseinds = R.noiseinds(pr)
    chain.noisepriors = [(pr["noise_lo"][i], pr["noise_hi"][i]) for i in range(2 * pr["nt"])]
    chain.iter_phase1, chain.iterations, chain.iiter = pr["iter_burnin"], pr["iterations"], iiter
    chain.modelmods = ['vsmod', 'zvmod', 'birth', 'death']
    chain.noisemods = [] if len(chain.noiseinds) == 0 else ['noise']
    chain.vpvsmods = [] if type(chain.priors['vpvs']) == np.float64 else ['vpvs']
    chain.modifications = chain.modelmods + chain.noisemods + chain.vpvsmods
    chain.propdist = np.array(st["propdist"], dtype=float)
    chain.proposed, chain.accepted = np.array(st["proposed"], dtype=float), np.array(st["accepted"], dtype=float)
    chain.currentmodel = np.concatenate((st["vs"], st["z"]))
    chain.currentnoise, chain.currentvpvs = np.array(st["noise"], dtype=float), np.float64(st["vpvs"])
    chain.currentlikelihood, chain.currentmisfits = np.float64(st["like"]), np.array(st["misfits"], dtype=float)
    chain.dvs2 = np.float64(0.0)
    chain.n, chain.tnull = 0, 0.0                      # (tnull: the status line `iterate` logs at iiter % 5000 == 0)
    chain.append_currentmodel = lambda: None           # (the sample store is sized for the chain's own targets)
    chain.targets = rec
    chain.rstate = InjectedRandomState()
    chain.rstate.set(d6)


def cases():
    rs = np.random.RandomState(2024)
    out = []
    for ML, nt in SHAPES:
        for r, pr0 in enumerate(R.records(nt, ML)):
            for iiter in ITERS:
                for absent in ((0, 1) if (r == 0 and iiter == 200) else (0,)):
                    pr = dict(pr0, absent=absent)
                    todo = [(st, d6) for _, st, d6, _ in R.crafted_propose(pr, iiter, rs)] if iiter in (-988, 200) else []
                    for k in range(6):
                        st = R.random_state(pr, rs, wide=bool(k % 2))
                        todo.append((st, np.concatenate((rs.uniform(size=5), rs.normal(size=1)))))
                    for st, d6 in todo:
                        fp = np.full(5, 50.0)
                        fp[4] = 0.0 if rs.uniform() < 0.2 else 50.0
                        st["proposed"], st["accepted"] = fp, np.minimum(fp, np.round(rs.uniform(0, 50, 5)))
                        if rs.uniform() < 0.3:
                            st["propdist"] = np.array([0.00104, 0.001, 0.002, 0.00105, 0.0010526])
                        out.append((pr, st, iiter, d6, st["like"] + 2.0 * rs.normal()))
    return out


def main():
    chain = make_chain()
    todo = cases()
    K = len(todo)
    o = dict(scalars=np.full((K, len(SCALARS)), np.nan), noise_lo=np.zeros((K, 2 * NTP)), noise_hi=np.zeros((K, 2 * NTP)),
             vs=np.zeros((K, MLP)), z=np.zeros((K, MLP)), noise=np.zeros((K, 2 * NTP)), draws=np.zeros((K, 6)),
             propdist=np.zeros((K, 5)), proposed=np.zeros((K, 5)), accepted=np.zeros((K, 5)),
             # recorded: move (-1: death of the only nucleus, the reference raises), valid, evaluated, accepted_flag, pn
             flags=np.zeros((K, 5), dtype=np.int32), pvs=np.zeros((K, MLP)), pz=np.zeros((K, MLP)), ph=np.zeros((K, MLP)),
             pvp=np.zeros((K, MLP)), pnoise=np.zeros((K, 2 * NTP)), pvpvs=np.zeros(K), dvs2=np.zeros(K), alpha=np.full(K, np.nan),
             propdist_out=np.zeros((K, 5)), proposed_out=np.zeros((K, 5)), accepted_out=np.zeros((K, 5)))
    for i, (pr, st, iiter, d6, newlike) in enumerate(todo):
        rec = Recorder()
        rec.like, rec.misfits = np.float64(newlike), np.zeros(pr["nt"] + 1)
        install(chain, pr, st, iiter, d6, rec)
        got = {}

        def wrap(name):
            f = getattr(type(chain), name)

            def g(*a, **k):
                got[name] = f(chain, *a, **k)
                got.setdefault("args_" + name, a)
                return got[name]
            setattr(chain, name, g)
        for name in ("_get_modelproposal", "_validmodel", "_get_hyperparameter_proposal", "_validnoise", "_get_vpvs_proposal",
                     "_validvpvs", "get_acceptance_probability"):
            wrap(name)
        n, nt = st["n"], pr["nt"]
        vals = dict(layermin=pr["layers"][0], layermax=pr["layers"][1], vsmin=pr["vs"][0], vsmax=pr["vs"][1], zmin=pr["z"][0],
                    zmax=pr["z"][1], thickmin=pr["thickmin"], lvz=np.nan if pr["lvz"] is None else pr["lvz"],
                    hvz=np.nan if pr["hvz"] is None else pr["hvz"], vpvsmin=pr["vpvs"][0], vpvsmax=pr["vpvs"][1],
                    mantle_vs=np.nan if pr["mantle"] is None else pr["mantle"][0],
                    mantle_vpvs=np.nan if pr["mantle"] is None else pr["mantle"][1], acc_lo=pr["acceptance"][0],
                    acc_hi=pr["acceptance"][1], iter_burnin=pr["iter_burnin"], iterations=pr["iterations"], iiter=iiter,
                    absent=pr["absent"], ML=pr["ML"], nt=nt, n=n, vpvs=st["vpvs"], like=st["like"], newlike=newlike)
        o["scalars"][i] = [vals[k] for k in SCALARS]
        o["noise_lo"][i, :2 * nt], o["noise_hi"][i, :2 * nt] = pr["noise_lo"], pr["noise_hi"]
        o["vs"][i, :n], o["z"][i, :n], o["noise"][i, :2 * nt] = st["vs"], st["z"], st["noise"]
        o["draws"][i], o["propdist"][i], o["proposed"][i], o["accepted"][i] = d6, st["propdist"], st["proposed"], st["accepted"]
        try:
            chain.iterate()
            raised = False
        except ValueError:                             # np.argmin of nothing: the death of the only nucleus
            raised = True
        if "args__get_modelproposal" in got:
            move = R.MOVES.index(got["args__get_modelproposal"][0])
        elif "_get_hyperparameter_proposal" in got:
            move = 4
        elif "_get_vpvs_proposal" in got:
            move = 5
        else:
            move = -1                                  # the death of the only nucleus: nothing returned
        valid = bool(got.get("_validmodel", got.get("_validnoise", got.get("_validvpvs", False)))) and not raised
        o["flags"][i] = (move, valid, rec.seen is not None, int(chain.accepted.sum() > st["accepted"].sum()), 0)
        if "_get_modelproposal" in got:
            m = got["_get_modelproposal"]
            pn = m.size // 2
            o["flags"][i, 4] = pn
            if pn <= MLP:
                o["pvs"][i, :pn], o["pz"][i, :pn] = m[:pn], m[pn:]
        o["dvs2"][i] = chain.dvs2
        if "_get_hyperparameter_proposal" in got:
            o["pnoise"][i, :2 * nt] = got["_get_hyperparameter_proposal"]
        if "_get_vpvs_proposal" in got:
            o["pvpvs"][i] = got["_get_vpvs_proposal"]
        if rec.seen is not None:
            h, vp, vs, noise = rec.seen
            o["ph"][i, :h.size], o["pvp"][i, :vp.size] = h, vp
            o["alpha"][i] = got["get_acceptance_probability"]
        o["propdist_out"][i], o["proposed_out"][i], o["accepted_out"][i] = chain.propdist, chain.proposed, chain.accepted
    path = os.path.join(HERE, "chain_step_golden.npz")
    np.savez_compressed(path, scalar_names=np.array(SCALARS), **o)
    print("%d cases, %d valid, %d accepted, %d B" % (K, int(o["flags"][:, 1].sum()), int(o["flags"][:, 3].sum()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
