"""The eval ride without a GPU: the descriptors HipBackend prepares on
``device="cpu"`` (the SelfTargetDesc of pass 0, the deferred EvalDesc), which fits
may carry an eval (HipBackend.eval_ride_ok), the driver's sequence on eligible
and ineligible runs (BackwardInduction.enqueue, checked with a proxy backend
that performs a handed-over eval inside ``fit``), the switch, and the torch
backend, which has no such route."""
import numpy as np
import pytest
import torch

from rphedge.models.hedge_mlp import NetSpec, init_weights
from rphedge.ops import layout as L

N = 1 << 12


def _hip(shape=(1, 8, 2, 0), world=1, **tc):
    from rphedge.engine import HipBackend, TrainConfig

    kw = dict(comm=object()) if world > 1 else {}
    return HipBackend(NetSpec(*shape), N, TrainConfig(batch_size=N, lm_gram_paths=2048, lm_out_fix=True, **tc),
                      device="cpu", world=world, **kw)


def _dates(nin=1):
    """(fit data of date t, eval data of date t+1): the eval's prices at its date are the fit's prices_next."""
    from rphedge.engine import DateData

    g = torch.Generator().manual_seed(3)
    x0 = [torch.rand(N, generator=g) + 0.5 for _ in range(nin)]
    x1 = [torch.rand(N, generator=g) + 0.5 for _ in range(nin)]
    p1, p2 = [x1[0] * 1.0], [x1[0] * 1.01]
    target = torch.zeros(N)
    fit = DateData(feats=x0, prices_next=p1, bond_next=1.01, target=target, fmu=tuple([0.9] * nin), fisd=tuple([3.0] * nin))
    ev = DateData(feats=x1, prices_next=p2, bond_next=1.02, target=torch.ones(N), prices_now=p1, bond_now=1.01,
                  fmu=tuple([0.8] * nin), fisd=tuple([2.0] * nin))
    return fit, ev


def _lm_cfg(**kw):
    from rphedge.engine import FitConfig

    return FitConfig(**dict(dict(optimizer="lm", epochs=1, early_stopping=False), **kw))


def test_descriptors_prepare_on_cpu():
    be = _hip()
    w, o, f = be.new_weights(init_weights(be.spec, [0.5, 0.5], seed=1)), be.new_opt(), be.new_fit()
    fit, ev = _dates()
    stats = be.new_stats()
    acc = torch.zeros(N)
    e = be.eval_desc(w, ev, stats, pnl_acc=acc, pnl_grow=1.01, pnl_carry=0.99, pnl_first=True)
    assert (e.v_out, e.wa, e.stats, e.pnl_acc, e.pnl_first) == (None, w.data_ptr(), stats.data_ptr(), acc.data_ptr(), 1)
    assert e.price_t[0] == fit.prices_next[0].data_ptr() and e.num_wgs == be.eval_wgs == N // 256
    d, lm, st = be._lm_prepare(w, o, f, fit, _lm_cfg(), ride=e)
    assert st.st_out == d.target == fit.target.data_ptr() and st.st_wts == w.data_ptr()
    assert st.st_feat[0] == ev.feats[0].data_ptr() and st.st_feat[1] is None
    assert (st.st_fmu[0], st.st_fisd[0]) == (np.float32(0.8), 2.0)
    # the self-target descriptor is the ride's own: the fit's shared LmDesc is the one of a fit without a ride
    blob = bytes(lm)
    d, lm2 = be._lm_prepare(w, o, f, fit, _lm_cfg())
    assert lm2 is lm and bytes(lm) == blob
    # ... and its layout is checked by name at load, in a table of its own
    from rphedge.ops import native
    rows = native.native_layout_ride(native.load(required=True))
    assert {t for t, *_ in rows} == {"SelfTargetDesc"} and len(rows) == len(native.SelfTargetDesc._fields_) == 5
    assert native.layout_mismatches(rows, [], classes=native.DESCRIPTORS_RIDE, layout=type("E", (), {})) == []
    # an eval of other prices, of two networks or with a v_out elsewhere is not this fit's target
    fit2, ev2 = _dates()
    with pytest.raises(ValueError, match="not this fit's prices_next"):
        be._lm_prepare(w, o, f, fit, _lm_cfg(), ride=be.eval_desc(w, ev2, stats))
    with pytest.raises(ValueError, match="one network"):
        be._lm_prepare(w, o, f, fit, _lm_cfg(), ride=be.eval_desc(w, ev, stats, wts_b=w))
    with pytest.raises(ValueError, match="one network"):
        be._lm_prepare(w, o, f, fit, _lm_cfg(), ride=be.eval_desc(w, ev, stats, v_out=acc))
    with pytest.raises(ValueError, match="cannot carry an eval"):
        be._lm_prepare(w, o, f, fit, _lm_cfg(lm_renorm=((0.3,), (2.0,))), ride=e)
    # riders: every free workgroup slot - two per CU where two of the solve's LDS images fit its 160 KB
    lds = be.native.lm_solve_lds(*be.shape)
    assert 0 < lds and be.eval_riders() == (2 if 2 * (lds + 4096) <= 160 * 1024 else 1) * 256 - L.LM_SPEC
    assert _hip((1, 32, 2, 0)).native.lm_solve_lds(1, 32, 2, 0) == 0


def test_which_fits_may_carry_an_eval():
    from rphedge.engine import FitConfig

    be = _hip()
    assert be.eval_ride_ok(_lm_cfg()) and be.eval_ride_ok(_lm_cfg(epochs=2, lm_lam_carry=3.0))
    assert _hip((2, 8, 2, 0)).eval_ride_ok(_lm_cfg())
    assert not be.eval_ride_ok(FitConfig(epochs=4))                              # Adam
    assert not be.eval_ride_ok(_lm_cfg(loss=L.LOSS_PINBALL, lm_q_delta=1e-3))    # the pension runs' pinball fits
    assert not be.eval_ride_ok(_lm_cfg(lm_renorm=((0.3,), (2.0,))))             # start-point transform
    assert not be.eval_ride_ok(_lm_cfg(epochs=0))                                # no trial point: pass 0 is the final body
    assert not be.eval_ride_ok(_lm_cfg(lm_starts=4, lm_explore_passes=2))        # a first date's exploration
    for shape in [(3, 8, 2, 0), (1, 8, 1, 1), (5, 8, 6, 0)]:                     # no self-target body (one wave per SIMD)
        assert not _hip(shape).eval_ride_ok(_lm_cfg()), shape
    assert not _hip((1, 32, 2, 0)).eval_ride_ok(_lm_cfg())                       # the wide nets have no LM solver
    assert not _hip(eval_ride=False).eval_ride_ok(_lm_cfg())                     # the switch
    assert not _hip(lm_split=True).eval_ride_ok(_lm_cfg())                       # pass / exchange / solve, one launch each
    assert not _hip(world=2).eval_ride_ok(_lm_cfg())


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
class _RideProxy:
    """The torch backend with the ride interface of HipBackend: ``eval_desc``
    records the eval, ``fit(ride=...)`` performs it (writing the fit's target)
    and then fits - what pass 0 and the first solve launch do on the GPU."""

    def __init__(self, inner, hip):
        self._inner, self._hip, self.log = inner, hip, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def eval_ride_ok(self, fcfg):
        return self._hip.eval_ride_ok(fcfg)

    def eval_desc(self, wts, data, stats, **kw):
        assert "v_out" not in kw
        self.log.append("defer")
        return (wts, data, stats, kw)

    def eval(self, *a, **kw):
        self.log.append("eval")
        return self._inner.eval(*a, **kw)

    def fit(self, wts, opt, fit, data, fcfg, seed, poll_every=0, ride=None):
        if ride is not None:
            w, ed, st, kw = ride
            self.log.append("fit+ride")
            self._inner.eval(w, ed, st, v_out=data.target, **kw)
        else:
            self.log.append("fit")
        return self._inner.fit(wts, opt, fit, data, fcfg, seed, poll_every)


def _params(**kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.25, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.25, n_paths=10, payoff="call", option_type="CALL", model="gbm_log", mortality=False, q99=False,
             optimizer="lm", lm_passes_first=6, lm_passes_rest=1, early_stopping=False, verbose=False, seed=1234,
             batch_size=1024, device="cpu", backend="torch")
    p.update(kw)
    return p


def _drive(proxy, **kw):
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(_params(**kw)))
    run.build()
    px = None
    if proxy:
        tc = {k: v for k, v in dict(eval_ride=kw.get("eval_ride", True)).items()}
        px = _RideProxy(run.backend, _hip(**tc))
        run.induction.backend = px
    res = run.run()
    return res, run.induction, px


def test_driver_hands_later_evals_to_the_next_fit():
    ref, ind0, _ = _drive(False)
    assert ind0.eval_rides == 0  # the torch backend has no such route
    res, ind, px = _drive(True)
    assert ind.n_dates == 4 and ind.eval_rides == 3
    assert px.log == ["fit", "defer", "fit+ride", "defer", "fit+ride", "defer", "fit+ride", "eval"]
    assert torch.equal(ind.values, ind0.values) and torch.equal(ind.snap, ind0.snap) and res.v0 == ref.v0
    for a, b in zip(ind.stats, ind0.stats):
        assert torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", ["switch", "adam", "renorm", "exercise", "pension", "cold_start"])
def test_driver_keeps_the_present_sequence(case):
    kw = dict(switch=dict(eval_ride=False), adam=dict(optimizer="adam", epochs_first=2, epochs_rest=1),
              renorm=dict(lm_renorm=True, feature_norm="date"),
              exercise=dict(payoff="put", option_type="PUT", exercise="bermudan", exercise_every=2),
              pension=dict(q99=True), cold_start=dict(warm_start=False))[case]
    _, ind, px = _drive(True, **kw)
    assert ind.eval_rides == 0 and "defer" not in px.log and "fit+ride" not in px.log
    assert px.log.count("eval") >= ind.n_dates
