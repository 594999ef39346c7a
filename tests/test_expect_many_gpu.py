"""``mpse_mps_expect_many`` on the GPU (``Engine.mps_expect_many``): chains of numpy arrays from a fixed seed and lists
of random MPO windows against the same contraction as ``numpy.einsum`` on the host, through the chain kernels and again
through the enqueued path (MPSE_EXPECT_CHAIN=0); ``took_path`` asserts which one ran.

Tolerance of a value: 1e-12 * prod_i |A_i|_F^2 * prod_{i in window} |W_i|_F.  Every transfer obeys |E'|_F <= |A|_F^2
|W|_F |E|_F (the bound tests/test_corr_gpu.py derives; the identity outside the window adds no factor beyond |A|_F^2),
so that product bounds the value, and the rounding of the at most 6 site steps and one closing sum, each a few hundred
FP64 products per entry, stays three orders of magnitude inside 1e-12 of it.  Every case prints its largest error /
scale before it asserts."""
import numpy as np
import pytest

from chain_problems import _chain, _dev, _rand, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

BONDS, DS = (1, 3, 7, 10, 5, 2, 1), (2, 3, 2, 4, 2, 3)
# (first, last, MPO bonds inside the window); (2, 3) twice: a shared pair of edges; None: the identity everywhere
WINDOWS = ((0, 0, ()), (5, 5, ()), (0, 5, (3, 8, 1, 8, 3)), (2, 3, (3,)), (1, 4, (8, 1, 3)), (3, 3, ()), (2, 3, (8,)),
           None)
KINDS = {"real": (False, True), "complex": (True, True), "mixed": ([False, False, True, True, False, False], True),
         "real_real_mpo": (False, False)}


def _window_mpo(rng, ds, first, last, inner, cplx):
    wb = (1,) + tuple(inner) + (1,)
    assert len(wb) == last - first + 2
    return first, [_rand(rng, (wb[j], ds[first + j], ds[first + j], wb[j + 1]), cplx) for j in range(last - first + 1)]


def _operators(rng, ds, windows, cplx):
    """[(first, [W of the window])]; the identity everywhere is a window of one identity site at site 0"""
    out = []
    for w in windows:
        if w is None:
            out.append((0, [np.eye(ds[0]).reshape(1, ds[0], ds[0], 1)]))
        else:
            out.append(_window_mpo(rng, ds, w[0], w[1], w[2], cplx))
    return out


def _host_value(sites, first, ws, conj=True, transpose_w=False):
    e = np.ones((1, 1, 1))
    for i, a in enumerate(sites):
        a4 = a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1])
        d = a4.shape[1]
        w = ws[i - first] if first <= i < first + len(ws) else np.eye(d).reshape(1, d, d, 1)
        if transpose_w:
            w = w.transpose(0, 2, 1, 3)
        e = np.einsum("bgk,bsac,gstu,ktad->cud", e, a4.conj() if conj else a4, w, a4, optimize=True)
    return complex(e[0, 0, 0])


def _host_reference(sites, operators):
    base = float(np.prod([np.linalg.norm(a) ** 2 for a in sites]))
    val = np.array([_host_value(sites, f, ws) for f, ws in operators])
    scale = np.array([base * np.prod([np.linalg.norm(w) for w in ws]) for _, ws in operators])
    return val, scale


def _check(eng, sites, operators, path, ref=None):
    """one call against numpy on the path the case means to take; returns (values, reference)"""
    if ref is None:
        ref = _host_reference(sites, operators)
    val, scale = ref
    dev = _dev(eng, sites)
    dev_ops = [(f, _dev(eng, ws)) for f, ws in operators]
    got, s0, s1 = took_path(eng.mps_expect_many_stats, lambda: eng.mps_expect_many(dev, dev_ops), path, len(sites))
    print(f"{path} {len(operators)} operators: max |value - numpy| / scale = {(np.abs(got - val) / scale).max():.2e}")
    assert s1["entries"] - s0["entries"] == len(operators)
    assert got.shape == val.shape and np.all(np.abs(got - val) <= 1e-12 * scale), (got, val)
    return got, ref


def _both_paths(eng, monkeypatch, sites, operators, first_path="chain_kernel"):
    a, ref = _check(eng, sites, operators, first_path)
    monkeypatch.setenv("MPSE_EXPECT_CHAIN", "0")
    b, _ = _check(eng, sites, operators, "enqueued", ref)
    monkeypatch.delenv("MPSE_EXPECT_CHAIN")
    assert np.all(np.abs(a - b) <= 2e-12 * ref[1])
    return a, b, ref


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


@pytest.mark.parametrize("kind", list(KINDS))
def test_windows_of_every_kind(eng, kind, monkeypatch):
    """all the windows in one call: both edges of the chain (the 1 x 1 sentinel), the whole chain, inner windows, a
    window given twice, the identity everywhere; MPO bonds 1, 3 and 8 (the channel limit)"""
    s_cplx, w_cplx = KINDS[kind]
    rng = np.random.default_rng(31)
    sites = _chain(rng, BONDS, DS, s_cplx)
    operators = _operators(rng, DS, WINDOWS, w_cplx)
    a, b, (val, scale) = _both_paths(eng, monkeypatch, sites, operators)
    norm = _host_value(sites, 0, [])
    assert abs(val[-1] - norm) <= 1e-13 * abs(norm)             # the identity everywhere is <psi|psi>
    assert abs(a[-1] - norm) <= 1e-12 * scale[-1]
    if kind == "real_real_mpo":
        assert np.all(a.imag == 0) and np.all(b.imag == 0)      # exactly zero, not small


def test_mpo_bond_over_the_channel_limit_is_enqueued(eng):
    rng = np.random.default_rng(32)
    sites = _chain(rng, BONDS, DS, True)
    operators = _operators(rng, DS, ((2, 3, (3,)), (1, 3, (8, 9)), (4, 4, ())), True)
    _check(eng, sites, operators, "enqueued")


def test_structurally_zero_rows(eng, monkeypatch):
    """MPO sites as ``Mpo.intersite`` gives them: pass-through channels and one-entry operators, most rows of W zero"""
    rng = np.random.default_rng(33)
    sites = _chain(rng, BONDS, DS, True)

    def site(wl, wr, d, entries):
        w = np.zeros((wl, d, d, wr))
        for (g, gp), m in entries.items():
            w[g, :, :, gp] = m
        return w

    def lower(d):
        return np.diag(np.sqrt(np.arange(1, d)), -1)

    # a^+ on site 1 ... a on site 4 with identities passed through channel 0 and a second, empty channel
    op1 = (1, [site(1, 2, 3, {(0, 0): lower(3)}), site(2, 2, 2, {(0, 0): np.eye(2)}), site(2, 2, 4, {(0, 0): np.eye(4)}),
               site(2, 1, 2, {(0, 0): lower(2).T})])
    # a sum of two terms in two channels, the second vanishing at its last site
    op2 = (3, [site(1, 2, 4, {(0, 0): lower(4), (0, 1): np.eye(4)}), site(2, 1, 2, {(0, 0): lower(2).T})])
    _both_paths(eng, monkeypatch, sites, [op1, op2])


def test_more_operators_than_one_launch(eng, monkeypatch):
    from renormalizer_amd.engine import mps_expect_many_plan
    cap = mps_expect_many_plan([[1, 2, 1, 1]], [(0, [(1, 1)])], True)[1]["grid_cap"]
    rng = np.random.default_rng(34)
    bonds, ds = (1, 2, 2, 1), (2, 2, 2)
    sites = _chain(rng, bonds, ds, True)
    kinds = ((0, 0, ()), (1, 2, (3,)), (0, 2, (2, 2)), (2, 2, ()))
    operators = _operators(rng, ds, [kinds[m % 4] for m in range(2 * cap + 3)], True)
    _both_paths(eng, monkeypatch, sites, operators)


@pytest.mark.parametrize("d, danc", ((2, 2), (2, 3)))
def test_density_operator_sites(eng, d, danc, monkeypatch):
    rng = np.random.default_rng(35)
    ds = (d,) * 3
    sites = _chain(rng, (1, 3, 4, 1), ds, [True, False, True], danc=(danc,) * 3)
    operators = _operators(rng, ds, ((0, 2, (3, 2)), (1, 1, ()), (1, 2, (8,)), (0, 0, ()), None), True)
    _both_paths(eng, monkeypatch, sites, operators)


@pytest.mark.parametrize("cplx", (False, True))
def test_state_bond_at_the_limit_and_above(eng, cplx, monkeypatch):
    """three sites with the inner bonds at the limit of the path rule and one above: the counters say which path ran;
    above the limit MPSE_EXPECT_CHAIN=1 sends the chain to the kernels as long as the launches fit"""
    from renormalizer_amd.engine import mps_expect_many_plan
    limit = mps_expect_many_plan([[1, 2, 1, 1]], [(0, [(1, 1)])], cplx)[1]["bond_limit"]
    rng = np.random.default_rng(36)
    ds = (2, 3, 2)
    for top, path, env in ((limit, "chain_kernel", None), (limit + 1, "enqueued", None), (limit + 1, "chain_kernel", "1")):
        bonds = (1, top, top, 1)
        operators = _operators(rng, ds, ((0, 2, (2, 2)), (1, 1, ()), (1, 2, (3,)), None), cplx)
        wins = [(f, [(w.shape[0], w.shape[3]) for w in ws]) for f, ws in operators]
        ok, info = mps_expect_many_plan([[bonds[i], ds[i], 1, bonds[i + 1]] for i in range(3)], wins, cplx)
        if env is not None:
            if info["lds_fit_bytes"] == 0:
                continue                                          # the limit is all that fits: nothing above it to run
            monkeypatch.setenv("MPSE_EXPECT_CHAIN", env)
        else:
            assert ok == (path == "chain_kernel")
        sites = [a / np.sqrt(a.size) for a in _chain(rng, bonds, ds, cplx)]
        _check(eng, sites, operators, path)
        monkeypatch.delenv("MPSE_EXPECT_CHAIN", raising=False)


def test_slots_are_not_interchangeable():
    """the references with transposed W, with an unconjugated bra and with a window shifted lie far outside the
    tolerance of the one asked for: the checks above can tell them apart (host arrays only).  Neighbouring sites of
    this chain differ in d, so a window is shifted to the next site of its own d: by two sites, or four.  The windows
    are those of at most two sites: over the four and six random sites of (1, 4) and (0, 5) the Frobenius product of
    the scale is so loose that the values themselves are 1e-7 of it (every seed tried), and no two references can lie
    1e-6 of it apart."""
    rng = np.random.default_rng(31)
    sites = _chain(rng, BONDS, DS, True)
    operators = _operators(rng, DS, [w for w in WINDOWS[:-1] if w[1] - w[0] < 2], True)
    assert len(operators) == 5
    for f, ws in operators:
        ref = _host_value(sites, f, ws)
        sc = float(np.prod([np.linalg.norm(a) ** 2 for a in sites]) * np.prod([np.linalg.norm(w) for w in ws]))
        assert abs(_host_value(sites, f, ws, transpose_w=True) - ref) > 1e-6 * sc
        assert abs(_host_value(sites, f, ws, conj=False) - ref) > 1e-6 * sc
    # d = 2 at the sites 0, 2 and 4, d = 3 at 1 and 5
    for f, g in ((0, 2), (2, 4), (1, 5)):
        w = _rand(rng, (1, DS[f], DS[f], 1), True)
        sc = float(np.prod([np.linalg.norm(a) ** 2 for a in sites]) * np.linalg.norm(w))
        assert abs(_host_value(sites, f, [w]) - _host_value(sites, g, [w])) > 1e-6 * sc
