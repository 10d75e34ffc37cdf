"""The sim ride without a GPU: the slice schedule of the rider blocks (the
native sim_ride_slice, the function the launcher and the riders use), the
SimRideDesc layout table, which first-date fits may carry the run's path scan
(HipBackend.sim_ride_ok, BackwardInduction.sim_ride_ok), the descriptor
HedgeRun prepares without a launch, the hand-over to the first date's fit and
the guard that finishes a split simulation nobody carried."""
import ctypes as C

import pytest
import torch

from rphedge.models.hedge_mlp import NetSpec
from rphedge.ops import layout as L

N = 1 << 12


def _hip(shape=(1, 8, 2, 0), world=1, **tc):
    from rphedge.engine import HipBackend, TrainConfig

    kw = dict(comm=object()) if world > 1 else {}
    return HipBackend(NetSpec(*shape), N, TrainConfig(batch_size=N, lm_gram_paths=2048, lm_out_fix=True, **tc),
                      device="cpu", world=world, **kw)


def _cfg(**kw):
    from rphedge.engine import FitConfig

    return FitConfig(**dict(dict(optimizer="lm", epochs=3, early_stopping=False, lm_starts=4, lm_explore_passes=5,
                                 lm_explore_paths=1024), **kw))


# ---------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("b0,b1,riders,per", [(4, 32, 3, 1), (4, 32, 7, 1), (4, 33, 7, 2), (0, 5, 448, 1),
                                              (128, 4096, 448, 1), (128, 4096, 192, 3), (7, 8, 1, 1), (5, 5, 9, 2)])
def test_every_block_rides_exactly_once(b0, b1, riders, per):
    from rphedge.ops import native

    seen, k, nxt = [], 0, b0
    while True:
        start, count = native.sim_ride_slice(b0, b1, riders, per, k)
        assert start == nxt and 0 <= count <= riders * per and start + count <= b1
        if count == 0:
            break
        # the riders' walk (k_lm_solve_sim): rider r takes start + r + j * riders, j < per, below the slice's end
        for r in range(riders):
            seen += [start + r + j * riders for j in range(per) if r + j * riders < count]
        nxt, k = start + count, k + 1
    assert sorted(seen) == list(range(b0, b1)) and nxt == b1
    assert k == -(-(b1 - b0) // (riders * per))
    # a launcher that runs out of solves after m launches sends [next, b1) out plainly: nothing twice, nothing lost
    for m in range(k + 1):
        s, c = native.sim_ride_slice(b0, b1, riders, per, m)
        assert s == min(b1, b0 + m * riders * per)


def test_layout_table_of_its_own():
    from rphedge.ops import native

    rows = native.native_layout_sim(native.load(required=True))
    assert {t for t, *_ in rows} == {"SimRideDesc"} and len(rows) == len(native.SimRideDesc._fields_)
    assert native.layout_mismatches(rows, [], classes=native.DESCRIPTORS_SIM, layout=type("E", (), {})) == []
    assert rows[0][1:] == ("sim", 0, C.sizeof(native.SimDesc))
    # the earlier tables keep their rows
    assert [c.__name__ for c in native.DESCRIPTORS_EXT] == ["OosDesc"]
    assert [c.__name__ for c in native.DESCRIPTORS_RIDE] == ["SelfTargetDesc"]


# ---------------------------------------------------------------------------
# eligibility
# ---------------------------------------------------------------------------
def test_which_fits_may_carry_the_scan(monkeypatch):
    from rphedge.engine import FitConfig

    be = _hip()
    assert be.sim_ride_ok(_cfg()) and be.sim_ride_ok(_cfg(lm_starts=1))        # (lm_explore_one: one start explores too)
    assert be.sim_ride_ok(_cfg(), L.SIM_GBM_LOG, 0) and be.sim_ride_ok(_cfg(), L.SIM_GBM_ARITH, 0)
    assert _hip((1, 8, 1, 1)).sim_ride_ok(_cfg(), L.SIM_GBM_LOG, 0)
    assert _hip((2, 8, 2, 0)).sim_ride_ok(_cfg(), L.SIM_HESTON, 0)
    assert not be.sim_ride_ok(_cfg(), L.SIM_HESTON, 0)                         # no rider: Heston's nets take two inputs
    assert not be.sim_ride_ok(_cfg(), L.SIM_GBM_LOG, L.STAT_MEAN)              # no rider: scans with a path statistic
    assert not _hip((2, 8, 2, 0)).sim_ride_ok(_cfg(), L.SIM_GBM_LOG, L.STAT_MAX)
    assert not be.sim_ride_ok(_cfg(), L.SIM_BASKET, 0) and not be.sim_ride_ok(_cfg(), L.SIM_MORTALITY, 0)
    assert not _hip((2, 8, 2, 0)).sim_ride_ok(_cfg(), L.SIM_SV_REF, 0)
    assert not be.sim_ride_ok(FitConfig(epochs=4))                              # Adam
    assert not be.sim_ride_ok(_cfg(lm_explore_passes=0))                        # no exploration
    assert not be.sim_ride_ok(_cfg(loss=L.LOSS_PINBALL, lm_q_delta=1e-3))
    assert not be.sim_ride_ok(_cfg(lm_explore_data=object()))                   # a prefix of other paths
    assert not _hip((1, 32, 2, 0)).sim_ride_ok(_cfg())                          # the wide nets have no LM solver
    assert not _hip(sim_ride=False).sim_ride_ok(_cfg())                         # the switch
    assert not _hip(lm_split=True).sim_ride_ok(_cfg())                          # pass / exchange / solve, one launch each
    assert not _hip(world=2).sim_ride_ok(_cfg())
    monkeypatch.setenv("RPH_SIM_RIDE", "0")
    assert not be.sim_ride_ok(_cfg())


def test_one_rider_per_cu_the_solves_leave(monkeypatch):
    be = _hip()
    assert be.sim_ride_steps() == 32 and be.sim_ride_blocks() == 1
    for K in (1, 4, 16):
        assert be.sim_riders(K) == 256 - K * L.LM_SPEC
    assert be.sim_riders(64) == 1 and be.sim_riders(80) == 1  # (never none: the launcher needs a rider)
    monkeypatch.setenv("RPH_SIM_RIDERS", "7")
    assert be.sim_riders(16) == 7


# ---------------------------------------------------------------------------
# HedgeRun: descriptor, hand-over, guard
# ---------------------------------------------------------------------------
def _params(**kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.25, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.25, n_paths=12, payoff="call", option_type="CALL", model="gbm_log", mortality=False, q99=False,
             optimizer="lm", lm_passes_first=4, lm_passes_rest=1, early_stopping=False, verbose=False, seed=1234,
             batch_size=N, device="cpu", backend="torch", lm_starts=4, lm_explore_passes=3, lm_explore_log2=10,
             keep_paths=False)
    p.update(kw)
    return p


class _Proxy:
    """The torch backend with HipBackend's sim ride interface: ``fit`` logs a handed-over ride."""

    def __init__(self, inner, hip):
        self._inner, self._hip, self.log = inner, hip, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def sim_ride_ok(self, fcfg, model=None, path_stat=0):
        return self._hip.sim_ride_ok(fcfg, model, path_stat)

    def lm_explore_paths(self, fcfg):
        return self._hip.lm_explore_paths(fcfg)

    def sim_ride_steps(self):
        return self._hip.sim_ride_steps()

    def sim_ride_blocks(self):
        return self._hip.sim_ride_blocks()

    def fit(self, wts, opt, fit, data, fcfg, seed, poll_every=0, ride=None, sim_ride=None):
        self.log.append("fit" if sim_ride is None else ("fit+sim", sim_ride))
        return self._inner.fit(wts, opt, fit, data, fcfg, seed, poll_every)


def _run(**kw):
    """A built CPU run that believes its backend is HipBackend (proxy), and the scan descriptor of its paths."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.ops import native

    run = HedgeRun(parse_params(_params(**kw)))
    run.build()
    px = _Proxy(run.backend, _hip((run.spec.nin, run.spec.hidden, run.spec.nout, run.spec.head),
                                  sim_ride=kw.get("sim_ride", True)))
    run.backend = run.induction.backend = px
    run.backend_kind = "hip"
    d = native.SimDesc()
    d.model, d.n_local, d.path_offset, d.final_out, d.out, d.n_fine = L.SIM_GBM_LOG, N, 0, 0x1000, 0x2000, 31
    return run, px, d


def test_descriptor_without_a_launch():
    run, px, d = _run()
    r = run._sim_ride_desc(d)
    assert r is not None and (r.b0, r.b1, r.per_rider, r.pay_kind) == (1024 // 256, N // 256, 1, 1)
    assert r.pay_out == run.v_terminal.data_ptr() and r.pay_out2 == run.induction.values[-1].data_ptr()
    assert r.strike == 1.0 and bytes(r.sim) == bytes(d) and C.addressof(r.sim) != C.addressof(d)
    # what keeps today's sequence: fp64, a mapped or unaligned scan, no fine terminal value, a path statistic,
    # a scan with no rider under this net, a scan too long to end with a solve (33 points; 32 still ride)
    ok = type(d).from_buffer_copy(d)
    ok.n_fine = 33
    assert run._sim_ride_desc(ok) is not None
    # the Gram subsample's scan rides in the head launch: it must select the same kernel
    g = type(d).from_buffer_copy(d)
    g.n_local, g.map_blk, g.map_stride = 512, 64, 1024
    assert run._sim_ride_desc(d, g) is not None
    for field, val in [("model", L.SIM_GBM_ARITH), ("fp64", 1), ("n_local", 500), ("map_stride", 1000)]:
        bad = type(g).from_buffer_copy(g)
        setattr(bad, field, val)
        assert run._sim_ride_desc(d, bad) is None, field
    for field, val in [("fp64", 1), ("map_blk", 64), ("n_local", N - 1), ("path_offset", 32), ("final_out", None),
                       ("path_stat", L.STAT_MEAN), ("model", L.SIM_HESTON), ("n_fine", 34)]:
        bad = type(d).from_buffer_copy(d)
        setattr(bad, field, val)
        assert run._sim_ride_desc(bad) is None, field
    # ... an exploration that reads every block, per-path reports, two networks, Adam, one start, the switch
    assert _run(lm_explore_log2=12)[0]._sim_ride_desc(d) is None
    for kw in [dict(keep_paths=True), dict(q99=True), dict(optimizer="adam", epochs_first=2, epochs_rest=1),
               dict(lm_starts=1), dict(sim_ride=False)]:
        run2, _, d2 = _run(**kw)
        assert run2._sim_ride_desc(d2) is None, kw
    run3, _, d3 = _run(payoff="put", option_type="PUT")
    assert run3._sim_ride_desc(d3).pay_kind == 2
    # before build() there is no values row to write
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    assert HedgeRun(parse_params(_params()))._sim_ride_desc(d) is None


def test_enqueue_hands_the_ride_to_the_first_fit_only():
    run, px, d = _run()
    r = run._sim_ride_desc(d)
    run.sim_ride = r
    before = run.induction.values[-1].clone().fill_(7.0)
    run.induction.values[-1].copy_(before)  # (the ride's kernels write this row: enqueue must not copy over it)
    run.enqueue()
    assert run.sim_ride is None and px.log[0] == ("fit+sim", r) and px.log[1:] == ["fit"] * (run.induction.n_dates - 1)
    assert torch.equal(run.induction.values[-1], before)
    # without a pending ride: the copy, plain fits
    px.log.clear()
    run.enqueue()
    assert px.log == ["fit"] * run.induction.n_dates and torch.equal(run.induction.values[-1], run.v_terminal)
    with pytest.raises(ValueError, match="first date"):
        run.induction.enqueue(start=run.induction.n_dates - 2, sim_ride=r)


@pytest.mark.parametrize("reader", ["collect", "simulate", "out_of_sample", "resume", "flush"])
def test_guard_finishes_a_ride_nobody_carried(monkeypatch, reader):
    from rphedge.ops import native

    run, px, d = _run()
    run.enqueue()
    calls = []
    monkeypatch.setattr(native, "sim_ride_rest", lambda r, start=None, stream=None: calls.append((r, start)))
    r = run.sim_ride = run._sim_ride_desc(d)
    run.backend_kind = "torch"  # (the readers below run on the CPU backend)
    if reader == "collect":
        run.collect()
    elif reader == "simulate":
        run.simulate()
    elif reader == "out_of_sample":
        monkeypatch.setattr("rphedge.oos.out_of_sample", lambda *a, **k: "oos")
        assert run.out_of_sample() == "oos"
    elif reader == "resume":
        # (the ride is finished before the saved date is even read)
        def stop(*a, **k):
            assert calls == [(r, None)]
            raise FileNotFoundError("no saved run")
        monkeypatch.setattr("rphedge.utils.model_io.load_date", stop)
        with pytest.raises(FileNotFoundError):
            run.resume("nowhere", 2)
    else:
        run.flush_sim_ride()
    assert calls == [(r, None)] and run.sim_ride is None
    run.flush_sim_ride()
    assert len(calls) == 1
