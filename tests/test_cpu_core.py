"""CPU tests: host twins of the device math, config/API plumbing, CPU engine."""
import ctypes
import math

import numpy as np
import pytest
import torch


def test_philox_known_answer():
    from rphedge.ops.philox import philox4x32_10

    r = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in r] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    m = 0xFFFFFFFF
    r = philox4x32_10(m, m, m, m, m, m)
    assert [int(v) for v in r] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("n", [1, 7, 64, 100, 4096])
def test_chunk_perm_is_bijection(n):
    from rphedge.ops.philox import ChunkPerm

    p = ChunkPerm(n, seed=11, epoch=3)
    y = p(np.arange(n))
    assert sorted(y.tolist()) == list(range(n))


def test_epoch_order_chunks():
    from rphedge.ops.philox import epoch_order

    o = epoch_order(4096, 6, 5, 0)
    assert sorted(o.tolist()) == list(range(4096))
    # chunks of 64 stay contiguous
    assert np.all(np.diff(o.reshape(-1, 64), axis=1) == 1)


def test_ndtri_twins_vs_scipy():
    from scipy.special import ndtri

    from rphedge.ops.ndtri import ndtri_u30_f32, ndtri_u30_f64

    rng = np.random.default_rng(0)
    x = np.concatenate([rng.integers(1, 2 ** 30, 50000), np.arange(1, 500), 2 ** 30 - np.arange(1, 500)])
    ref = ndtri(x * 2.0 ** -30)
    np.testing.assert_allclose(ndtri_u30_f64(x), ref, rtol=1e-12, atol=1e-13)
    core = np.abs(ref) < 5
    np.testing.assert_allclose(ndtri_u30_f32(x)[core], ref[core], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("d,m,seed", [(5, 8, 1235), (40, 10, 1234)])
def test_sobol_cpu_bit_exact(d, m, seed):
    from scipy.stats import qmc

    from rphedge.ops.sobol import sobol_uniform_cpu

    ref = qmc.Sobol(d, scramble=True, seed=seed).random_base2(m)
    assert np.array_equal(sobol_uniform_cpu(m, d, seed), ref)


def test_sobol_norm_api_cpu():
    from scipy.stats import norm, qmc

    from rphedge import sobol_norm

    z = sobol_norm(6, 3, 1235, device="cpu").numpy()
    ref = norm.ppf(qmc.Sobol(3, scramble=True, seed=1235).random_base2(6))
    np.testing.assert_allclose(z, ref, rtol=1e-12, atol=1e-13)


def test_native_layout_loads_without_gpu():
    from rphedge.ops import native

    lib = native.load(required=False)
    assert lib is not None
    assert native.net_nparams(3, 8, 2, 0) == (122, 128)
    assert native.net_nparams(1, 8, 1, 1) == (97, 128)


@pytest.fixture(scope="module")
def native_tables():
    from rphedge.ops import native

    return native.native_layout(native.load(required=False))


def _mirror(cls, edit):
    """A copy of the ctypes mirror ``cls`` with ``edit`` applied to its field list."""
    fields = list(cls._fields_)
    edit(fields, [f[0] for f in fields].index)
    return type(cls.__name__, (ctypes.Structure,), {"_fields_": fields})


def _swap(a, b):
    def edit(fields, at):
        fields[at(a)], fields[at(b)] = fields[at(b)], fields[at(a)]
    return edit


def _drop(name):
    return lambda fields, at: fields.pop(at(name))


def _retype(name, ctype):
    def edit(fields, at):
        fields[at(name)] = (name, ctype)
    return edit


def test_native_field_table_is_complete_and_matches(native_tables):
    from rphedge.ops import native

    fields, consts = native_tables
    assert len(fields) == sum(len(c._fields_) for c in native.DESCRIPTORS) == 215 + 8
    assert native.layout_mismatches(fields, consts) == []
    assert [ctypes.sizeof(c) for c in native.DESCRIPTORS] == [536, 480, 72, 384, 96, 488, 1032]


MUTATIONS = {
    "swap n_local/batch": ("TrainDesc", _swap("n_local", "batch"), ["n_local", "batch"]),
    "swap out2/out3": ("SimDesc", _swap("out2", "out3"), ["out2", "out3"]),
    "swap world/rank": ("LmDpDesc", _swap("world", "rank"), ["world", "rank"]),
    "drop lam_up": ("LmDesc", _drop("lam_up"), ["lam_up"]),
    "float to double": ("EvalDesc", _retype("hold_c", ctypes.c_double), ["hold_c"]),
    "drop pad_acc": ("TrainDesc", _drop("pad_acc"), ["pad_acc"]),   # (no offset moves: the hole comes back)
    "drop pad4": ("LmDesc", _drop("pad4"), ["pad4"]),               # (nor does the size: tail alignment)
}


@pytest.mark.parametrize("case", MUTATIONS)
def test_layout_comparison_names_a_wrong_mirror(native_tables, case):
    from rphedge.ops import native

    struct, edit, named = MUTATIONS[case]
    fields, consts = native_tables
    classes = tuple(_mirror(c, edit) if c.__name__ == struct else c for c in native.DESCRIPTORS)
    bad = native.layout_mismatches(fields, consts, classes=classes)
    for f in named:
        assert any(line.startswith(f"{struct}.{f}: ") for line in bad), (f, bad)
    assert all(line.startswith(struct) for line in bad), bad   # (no other struct is blamed)
    assert native.layout_mismatches(fields, consts) == []      # (the module's own mirrors are untouched)


def test_layout_comparison_names_a_wrong_constant(native_tables):
    import types

    from rphedge.ops import layout, native

    fields, consts = native_tables

    def bad(**edit):
        ns = dict(vars(layout))
        for k, v in edit.items():
            ns.pop(k) if v is None else ns.__setitem__(k, v)
        return native.layout_mismatches(fields, consts, layout=types.SimpleNamespace(**ns))

    assert bad() == []
    out = bad(LM_OUTG_TAIL=2)
    assert len(out) == 1 and out[0].startswith("layout.LM_OUTG_TAIL:") and "native 1" in out[0] and "python 2" in out[0]
    out = bad(ES_TAU=None)
    assert len(out) == 1 and out[0].startswith("layout.ES_TAU:") and "native 29" in out[0]
    out = bad(NEW_KNOB=7)
    assert len(out) == 1 and out[0].startswith("layout.NEW_KNOB:") and "not in the native table" in out[0]


def test_native_constants_resolve_in_layout(native_tables):
    from rphedge.ops import layout, native

    names = [n for n, _ in native_tables[1]]
    assert len(names) == len(set(names))
    assert [n for n in names if not isinstance(getattr(layout, n, None), int)] == []
    assert [n for n in native.PYTHON_ONLY if n in names] == []
    assert all(isinstance(getattr(layout, n), int) for n in native.PYTHON_ONLY)
    # the copies that used to live elsewhere are the layout module's
    import rphedge.engine as E

    assert (native.MAXIN, native.MAXHOLD, native.DP_SLOTS) == (layout.MAXIN, layout.MAXHOLD, layout.DP_SLOTS)
    assert E.MAXIN == layout.MAXIN == 8 and E.PNL_PPT == layout.PNL_PPT == 4


def test_param_counts_match_reference():
    from rphedge.models import EUROPEAN_REF, PENSION

    assert PENSION.nparams == 122       # "Multi Time Step.ipynb":617
    assert EUROPEAN_REF.nparams == 97   # "European Options.ipynb":451


def test_grid_matches_reference():
    from rphedge.ops.paths import Grid

    g = Grid(10.0, 1 / 100, 0.25)
    assert (g.n_fine, g.reduction, g.n_coarse) == (1001, 25, 41)
    g = Grid(10.0, 1 / 365, 0.25)
    assert (g.n_fine, g.reduction, g.n_coarse) == (3651, 91, 41)
    g = Grid(1.0, 1 / 365, 1 / 52)
    assert (g.n_fine, g.reduction, g.n_coarse) == (366, 7, 53)


def test_parse_params_keys():
    from rphedge.config import parse_params

    base = dict(Y=1, K=1, T=10, mu=0.09464, r=0.03, sigma=0.15965, rebalancing=0.25, N=10000, P=100, x=55,
                l0=0.01, c=0.075, ita=0.000597, dt=1 / 100, n_paths=12)
    cfg = parse_params(base)
    assert cfg.paths == 4096 and cfg.n_coarse == 41
    with pytest.raises(KeyError):
        parse_params({k: v for k, v in base.items() if k != "ita"})
    with pytest.raises(KeyError):
        parse_params(dict(base, bogus=1))
    sv = dict(base)
    sv.pop("sigma")
    sv.update(s0=0.15965, a=0.0033566, b=0.15431)
    cfg = parse_params(dict(sv, parity=True), sv=True)
    assert cfg.sv_c == 0.075 and cfg.model == "sv_ref"   # Q4


def test_gbm_cpu_moments():
    from rphedge.ops import paths as P

    g = P.Grid(10.0, 1 / 100, 0.25)
    p = P.simulate_gbm(g, 4096, 1.0, 0.09464, 0.15965, device="cpu")
    # MTS sanity check: mean Y_T ~ e^{mu T}
    assert abs(float(p.S_final.double().mean()) - math.exp(0.9464)) < 0.03


def test_black_scholes_reference_numbers():
    from rphedge.utils.reports import black_scholes

    price, delta = black_scholes(100, 100, 0.08, 0.15, 1.0)
    assert price == pytest.approx(10.3896, abs=1e-3)
    assert delta == pytest.approx(0.7285, abs=1e-3)


def test_cpu_quantile_exact():
    from rphedge import risk

    x = torch.randn(5001, generator=torch.Generator().manual_seed(3))
    qs = (0.0, 0.1, 0.5, 0.985, 1.0)
    np.testing.assert_allclose(risk.quantile(x, qs), np.quantile(x.double().numpy(), qs), rtol=1e-6, atol=1e-7)


def test_european_cpu_end_to_end():
    import rphedge

    res = rphedge.european_option(N_paths=4096, rebalancing_frequency=1 / 12, epochs_first=60, epochs_rest=15,
                                  verbose=False, batch_size=512)
    assert abs(res.v0 - 10.39) < 0.6
    assert abs(res.phi - 0.7285) < 0.08
    assert res.terminal_pnl["std"] < 3.5


def test_launcher_rejects_bad_descriptors():
    """Host-side validation in the native launchers (csrc/hedge_core.h
    validate_train): a malformed descriptor never reaches the GPU — checked
    here on CPU, where the library loads but no kernel may run."""
    from rphedge.ops import native

    native.load(required=True)
    d = native.TrainDesc()
    d.nin, d.h, d.nout, d.head = 1, 8, 2, 0
    d.num_wgs, d.batch, d.n_local, d.steps_per_epoch = 0, 512, 4096, 8
    with pytest.raises(RuntimeError, match="num_wgs"):
        native.train_step(d, 0, 0, stream=0)
    d.num_wgs = 16
    d.steps_per_epoch = 2  # 2 x 512 < 4096
    with pytest.raises(RuntimeError, match="batch"):
        native.train_lag_step(d, 0, 0, stream=0)
    d.steps_per_epoch = 8
    d.alpha = 1.5  # the kernels compute LeakyReLU as max(z, alpha z)
    with pytest.raises(RuntimeError, match="slope"):
        native.train_lag_fit(d, 1, stream=0)
    d.alpha = 0.3
    with pytest.raises(RuntimeError, match="null state"):
        native.train_fit(d, 1, stream=0)
    # dummy (never dereferenced) pointers past the null checks
    d.wts = d.opt = d.fit = d.target = d.feat[0] = 4096
    d.fisd[0] = 0.0
    with pytest.raises(RuntimeError, match="standardisation"):
        native.train_fit(d, 1, stream=0)
    d.fisd[0], d.fmu[0] = 1.0, float("nan")
    with pytest.raises(RuntimeError, match="standardisation"):
        native.train_lag_fit(d, 1, stream=0)


def test_launchers_reject_path_ranges_past_the_sobol_table():
    """The Sobol tables are 30-bit: rph_simulate / rph_sobol_normal report a
    range whose largest global index is >= 2^30 before any launch, and accept
    the ranges that end exactly on 2^30 - 1 (the dry-run entry points run the
    launchers' checks alone, so nothing is launched here either way)."""
    from rphedge.ops import layout as L
    from rphedge.ops import native
    from rphedge.ops import paths as P
    from rphedge.ops.paths import path_indices

    native.load(required=True)
    end = 1 << 30
    g = P.Grid(1.0, 1 / 32, 1 / 8)

    def desc(n, offset, index_map=None, model=L.SIM_HESTON):
        return P._desc(model, n, offset, g, False, False, index_map)

    # the exact fits: aligned, unaligned, and a map whose last block ends on the last index
    fits = [(512, end - 512, None), (300, end - 300, None), (1, end - 1, None), (2048, 0, None),
            (512, end - 7 * 1024 - 64, (64, 1024)), (300, end - 5 * 1000 - 50, (50, 1000))]
    for n, off, m in fits:
        assert int(path_indices(n, off, m).max()) == (end - 1 if off else n - 1)
        native.simulate_check(desc(n, off, m))
        native.simulate_check(desc(n, off, m, model=L.SIM_BASKET))
        if m is None:
            native.sobol_normal_check(n, off)
    # one past, far past, negative, and maps that leave the table only through the stride
    past = [(512, end - 511, None), (300, end - 299, None), (1, end, None), (1, 1 << 40, None), (256, -64, None),
            (512, end - 7 * 1024 - 63, (64, 1024)), (300, end - 5 * 1000 - 49, (50, 1000)),
            (128, 0, (64, end)), (192, 0, (64, 1 << 62))]
    for n, off, m in past:
        with pytest.raises(RuntimeError, match="30-bit Sobol"):
            native.simulate_check(desc(n, off, m))
        with pytest.raises(RuntimeError, match="30-bit Sobol"):
            native.simulate(desc(n, off, m, model=L.SIM_BASKET), stream=0)  # (null pointers: returns before the launch)
        if m is None:
            with pytest.raises(RuntimeError, match="30-bit Sobol"):
                native.sobol_normal_check(n, off)
    with pytest.raises(RuntimeError, match="30-bit Sobol"):
        native.sobol_normal(torch.empty(300, 3), (torch.empty(0), torch.empty(0), 3), offset=end - 299, stream=0)
    # the pair launcher checks both descriptors
    with pytest.raises(RuntimeError, match="30-bit Sobol"):
        native.simulate_pair(desc(512, 0), desc(512, end - 511), stream=0)


def test_mortality_twin_normal_branch():
    """_cpu_mortality follows the kernel from 200 expected deaths per step on
    (rounded normal approximation); below it nothing changes: the n0 = 10000
    numbers are those of the inversion-only twin."""
    from rphedge.ops import paths as P

    lam = (0.01, 0.075, 0.000597)
    g = P.Grid(2.0, 1 / 100, 0.25)
    share = []
    nf, lm, nt = P._cpu_mortality(g, 515, *lam, 10000, False, 37, P.SEED_W2, 1234, False, branch_share=share)
    assert len(share) == g.n_fine - 1 and max(share) == 0.0
    n_t = np.rint(nt * 10000).astype(int)
    assert n_t[:8].tolist() == [9742, 9803, 9807, 9762, 9803, 9776, 9809, 9783] and int(n_t.sum()) == 5039909
    assert np.rint(nf[:, 3] * 10000).astype(int).tolist() == [10000, 9973, 9949, 9920, 9892, 9858, 9829, 9791, 9762]

    g = P.Grid(2.0, 0.25, 0.5)
    n0 = 100000
    share = []
    a = P._cpu_mortality(g, 512, *lam, n0, False, 37, P.SEED_W2, 1234, False, branch_share=share)
    b = P._cpu_mortality(g, 512, *lam, n0, False, 37, P.SEED_W2, 1234, False)
    assert share == [1.0] * (g.n_fine - 1)
    for x, y in zip(a, b):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    N = a[0] * n0
    assert np.all(np.abs(N - np.rint(N)) < 1e-6) and np.all(N >= 0) and np.all(N <= n0)
    assert np.all(np.diff(N, axis=0) <= 0) and np.all(a[2] * n0 <= N[-1] + 1e-6)
    # about N q = 250 deaths per quarter, sd 16: the survivors after two years
    assert abs(float((a[2] * n0).mean()) - n0 * math.exp(-0.01 * 2.16)) < 100
    share = []
    P._cpu_mortality(g, 512, *lam, 80000, False, 37, P.SEED_W2, 1234, False, branch_share=share)
    assert all(0.5 < s < 0.99 for s in share)   # N q ~ 200: both branches in every step


# shape (nin, h, nout, head) -> net_nparams (P, R), lm_shape (P, R, NBLK) or None, lm_pass_wps:
# the one shape table of csrc/hedge_core.h, pinned to the values before it became one table
SHAPE_TABLE = {
    (1, 8, 1, 1): ((97, 128), (97, 128, 10), 1),
    (1, 8, 2, 0): ((106, 128), (106, 128, 10), 2),
    (2, 8, 2, 0): ((114, 128), (114, 128, 10), 2),
    (3, 8, 2, 0): ((122, 128), (122, 128, 10), 1),
    (4, 8, 2, 0): ((130, 256), (130, 256, 15), 1),
    (5, 8, 6, 0): ((174, 256), (174, 256, 21), 1),
    (6, 8, 7, 0): ((191, 256), (191, 256, 21), 1),
    (1, 32, 1, 1): ((1153, 1280), None, 1),
    (1, 32, 2, 0): ((1186, 1280), None, 1),
    (2, 32, 2, 0): ((1218, 1280), None, 1),
    (3, 32, 2, 0): ((1250, 1280), None, 1),
    (5, 32, 6, 0): ((1446, 1536), None, 1),
}
UNKNOWN_SHAPES = [(7, 8, 2, 0), (4, 32, 2, 0), (1, 8, 1, 0), (3, 16, 2, 0)]


def test_shape_table_pinned():
    from rphedge.ops import native

    native.load(required=True)
    for shape, (pr, lm, wps) in SHAPE_TABLE.items():
        assert native.net_nparams(*shape) == pr, shape
        assert native.lm_shape(*shape) == lm, shape
        assert native.lm_pass_wps(*shape) == wps, shape
    for shape in UNKNOWN_SHAPES:
        with pytest.raises(ValueError):
            native.net_nparams(*shape)
        assert native.lm_shape(*shape) is None, shape
        assert native.lm_pass_wps(*shape) == 1, shape


@pytest.mark.parametrize("shape", UNKNOWN_SHAPES)
def test_unknown_shape_is_a_reported_error(shape):
    """A shape outside the table on an otherwise valid descriptor: every
    launcher reports it under its own name with the four shape numbers (no
    kernel is launched: the dispatch fails first), never a message left over
    from an earlier call."""
    from rphedge.engine import PNL_PPT
    from rphedge.ops import native

    native.load(required=True)
    nin, h, nout, head = shape
    numbers = f"nin {nin}, h {h}, nout {nout}, head {head}"
    buf = torch.zeros(16)
    p = buf.data_ptr()  # non-null, never dereferenced

    def stale():  # leave another launcher's validation message in the error buffer
        bad = native.TrainDesc()
        bad.nin, bad.h, bad.nout, bad.head = 1, 8, 2, 0
        bad.num_wgs, bad.batch, bad.n_local, bad.steps_per_epoch = 0, 512, 4096, 8
        with pytest.raises(RuntimeError, match="num_wgs"):
            native.train_step(bad, 0, 0, stream=0)

    def expect(who, call, text=numbers):
        stale()
        with pytest.raises(RuntimeError) as e:
            call()
        msg = str(e.value)
        assert who in msg and text in msg and "num_wgs" not in msg, msg

    d = native.TrainDesc()
    d.nin, d.h, d.nout, d.head = shape
    d.num_wgs, d.batch, d.n_local, d.steps_per_epoch = 16, 512, 4096, 8
    d.alpha, d.chunk_log2 = 0.3, 6
    d.wts = d.opt = d.fit = d.target = d.lag = d.acc = d.counter = d.slab = d.grad_out = p
    d.fused_update = 1
    for i in range(native.MAXIN):
        d.feat[i], d.fisd[i] = p, 1.0
    for k in range(native.MAXHOLD):
        d.price[k] = p
    expect("rph_train_step", lambda: native.train_step(d, 0, 0, stream=0))
    expect("rph_train_lag_step", lambda: native.train_lag_step(d, 0, 0, stream=0))
    expect("rph_train_lag_finalize", lambda: native.train_lag_finalize(d, 1, stream=0))
    expect("rph_train_update", lambda: native.train_update(d, 0, 0, stream=0))

    e = native.EvalDesc()
    e.nin, e.h, e.nout, e.head = shape
    e.wa = e.stats = p
    e.n_local, e.num_wgs, e.alpha = 4096, 16, 0.3
    for i in range(native.MAXIN):
        e.feat[i], e.fisd[i] = p, 1.0
    expect("rph_eval", lambda: native.eval_(e, stream=0))

    q = native.PnlDesc()
    q.nin, q.h, q.nout, q.head = shape
    q.snap = q.stats = q.payoff = q.fmu = q.fisd = q.bond = p
    q.n_local, q.n_dates, q.alpha = 4096, 2, 0.3
    q.num_wgs = (q.n_local + 256 * PNL_PPT - 1) // (256 * PNL_PPT)
    for i in range(native.MAXIN):
        q.feat[i], q.feat_ts[i] = p, q.n_local
    for k in range(native.MAXHOLD):
        q.price[k], q.price_ts[k] = p, q.n_local
    if shape == (1, 8, 1, 0):
        # one free holding is no hedge: rph_pnl's own validation (holdings >= 2)
        # rejects this descriptor before the dispatch, as it always did
        expect("rph_pnl", lambda: native.pnl(q, stream=0), text="bad P&L descriptor")
    else:
        expect("rph_pnl", lambda: native.pnl(q, stream=0))


def test_feature_norms_modes():
    """driver.feature_norms: per-date / pooled moments; degenerate spread
    (every path at S_0 on date 0) keeps unit scale; parity forces raw."""
    from rphedge.driver import feature_norms
    from rphedge.ops import paths as P

    g = P.Grid(1.0, 0.1, 0.1)
    p = P.simulate_gbm(g, 1 << 12, 1.0, 0.08, 0.2, device="cpu", scheme="log")
    assert feature_norms(p, "none") == []
    nd = feature_norms(p, "date")
    assert len(nd) == p.n_coarse - 1
    assert nd[0] == ((pytest.approx(1.0),), (1.0,))
    t = p.n_coarse - 2
    x = p.features(t)[0].double()
    assert nd[t][0][0] == pytest.approx(float(x.mean()), rel=1e-6)  # (fp32 Welford)
    assert nd[t][1][0] == pytest.approx(1.0 / float(x.std(unbiased=False)), rel=1e-6)
    gl = feature_norms(p, "global")
    assert all(v == gl[0] for v in gl) and gl[0][1][0] > 1.0
    with pytest.raises(ValueError):
        feature_norms(p, "bogus")
    from rphedge.config import ParityFlags

    assert ParityFlags.reference().raw_features and not ParityFlags().raw_features


def test_feature_norms_horizon():
    """feature_norm="horizon": price inputs centred at the kink, scaled by the
    remaining-horizon spread m_t sd(log S_T - log S_t) (GBM: F_t sigma
    sqrt(T - t)) floored at floor x the date spread; the fixed-point moment
    sums make the scales independent of the path order (hence of the world
    size); Heston's variance input keeps the date scale."""
    from rphedge.driver import feature_norms
    from rphedge.ops import paths as P

    g = P.Grid(1.0, 0.1, 0.1)
    sig = 0.2
    p = P.simulate_gbm(g, 1 << 14, 1.0, 0.08, sig, device="cpu", scheme="log")
    nd = p.n_coarse - 1
    hz = feature_norms(p, "horizon", centers=(1.0,))
    dt = feature_norms(p, "date")
    tt = g.times()
    for t in range(nd):
        mu, isd = hz[t][0][0], hz[t][1][0]
        assert mu == 1.0                                     # the strike
        m = float(p.features(t)[0].double().mean())
        want = m * sig * math.sqrt(1.0 - tt[t])              # F_t sigma sqrt(T - t)
        assert 1.0 / isd == pytest.approx(want, rel=0.03), (t, 1.0 / isd, want)
    # the floor binds late: scale >= 0.5 x the date spread
    fl = feature_norms(p, "horizon", centers=(1.0,), floor=0.5)
    t = nd - 1
    assert 1.0 / fl[t][1][0] == pytest.approx(max(1.0 / hz[t][1][0], 0.5 / dt[t][1][0]), rel=1e-12)
    # order-independent (exact int64 sums): a permuted path set gives the same bits
    perm = torch.randperm(1 << 14, generator=torch.Generator().manual_seed(3))
    q = P.simulate_gbm(g, 1 << 14, 1.0, 0.08, sig, device="cpu", scheme="log")
    q.S = q.S[:, perm].contiguous()
    assert feature_norms(q, "horizon", centers=(1.0,)) == hz
    # Heston: the variance input keeps the date standardisation
    h = P.simulate_sv(g, 1 << 12, 1.0, 0.05, 0.04, model="heston", kappa=2.0, theta=0.04, xi=0.5, rho=-0.7,
                      device="cpu")
    hh, hd = feature_norms(h, "horizon", centers=(1.0, None)), feature_norms(h, "date")
    assert all(hh[t][0][1] == hd[t][0][1] and hh[t][1][1] == hd[t][1][1] for t in range(h.n_coarse - 1))
    assert hh[3][0][0] == 1.0 and hh[3][1][0] != hd[3][1][0]


def test_keras_adam_matches_torch_optim_adam_cpu():
    """Torch reference backend's Keras-Adam (K10 semantics) vs torch.optim.Adam
    for 3 full-batch steps; the per-step matching torch eps is eps/sqrt(1-b2^t)."""
    from rphedge.engine import DateData, FitConfig, TorchBackend, TrainConfig, current_weights
    from rphedge.models.hedge_mlp import NetSpec, init_weights

    spec = NetSpec(nin=1, hidden=8, nout=2, head=0)
    n = 1024
    x = torch.linspace(0.7, 1.3, n)
    w0 = init_weights(spec, [0.5, 0.0])
    lr, eps, b2 = 5e-3, 1e-7, 0.999
    be = TorchBackend(spec, n, TrainConfig(batch_size=n, lr=lr, eps=eps, shuffle=False), device="cpu",
                      dtype=torch.float64)
    data = DateData(feats=[x], prices_next=[x * 1.01], bond_next=1.0, target=torch.relu(x - 1), prices_now=[x])
    w, o, f = be.new_weights(w0), be.new_opt(), be.new_fit()
    be.fit(w, o, f, data, FitConfig(epochs=3, patience=10 ** 6, early_stopping=False), seed=1)
    wk = current_weights(spec, w)

    o_ = spec.offsets
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    X = x.double()[:, None]
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, b2), eps=eps)
    for t in range(1, 4):
        for gr in opt.param_groups:
            gr["eps"] = eps / math.sqrt(1 - b2 ** t)
        opt.zero_grad()
        a = torch.nn.functional.leaky_relu(X @ p[o_["W1"]:o_["b1"]].view(1, 8) + p[o_["b1"]:o_["W2"]], 0.3)
        a = torch.nn.functional.leaky_relu(a @ p[o_["W2"]:o_["b2"]].view(8, 8) + p[o_["b2"]:o_["W3"]], 0.3)
        h = a @ p[o_["W3"]:o_["b3"]].view(8, 2) + p[o_["b3"]:o_["P"]]
        V = h[:, 0] * (x.double() * 1.01) + h[:, 1]
        ((V - torch.relu(x.double() - 1)) ** 2).mean().backward()
        opt.step()
    np.testing.assert_allclose(wk, p.detach().numpy(), rtol=1e-5, atol=1e-7)
