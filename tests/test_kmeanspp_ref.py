"""CPU checks of the scripted k-means++ cases (tests/helpers/kmeanspp_ref.py) that tests/test_gpu_kmeanspp_edges.py runs on the
device: the cases reach the edges they are meant to reach (an inventory, so that none goes untested silently), on exact data
scikit-learn's own ``_kmeans_plusplus`` gives the oracle's indices from the same scripted draws, and the host half of the ABI
(trial count, workspace size, argument errors: all before any device call)."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import kmeanspp_ref as kr

NNC_OK, NNC_EINVAL, NNC_ENOSPACE = 0, -1, -2
SMALL = [c.name for c in kr.CASES if c.n <= 600_000]
ALL = [c.name for c in kr.CASES]
TARGET_TAGS = {"block_first", "block_last", "group_first_block", "group_last_block", "quarter0", "quarter1", "quarter2", "quarter3",
               "first_group", "last_group", "plateau_block0", "plateau_block-", "plateau_block+", "plateau_group0", "plateau_group-",
               "plateau_group+", "u_zero", "u_max", "equal_pair", "all_equal", "mirror", "rounding", "sample_fallback",
               "group0_first", "group63_last", "group64_first", "group64_above", "group64_mid"}


def _rounds(names):
    for name in names:
        b = kr.build(name)
        for rd in b.stepper.rounds:
            yield b, rd


def test_scripted_draws_hand_out_the_list_exactly():
    d = kr.ScriptedDraws(0.25, [0.5, 0.125, 0.75])
    assert d.choice(8) == 2 and d.uniform(size=2).tolist() == [0.5, 0.125]
    with pytest.raises(AssertionError):
        d.assert_consumed()
    assert d.uniform(size=1).tolist() == [0.75]
    d.assert_consumed()
    with pytest.raises(AssertionError):
        d.uniform(size=1)
    e = kr.ScriptedDraws(0.25, [])
    assert e.random_sample() == 0.25
    e.assert_consumed()
    for n in (1, 2, 5, 1025, 300_001):               # the first seed's index: the helper's closed form is the oracle's
        for u in (0.0, 0.37, kr.U_MAX, (n // 2 + 0.5) / n):
            assert orc.kmeans_plusplus(np.arange(n, dtype=np.float32), 1, kr.ScriptedDraws(u, []))[1][0] == kr.first_index(u, n)


def test_a_target_that_is_not_exact_is_refused():
    x, mean = kr.gaussian_data(3000, 9300)
    st = kr.Stepper((x - mean).astype(np.float32), 3, 0.4)
    refused = 0
    for j in range(0, 3000, 3):
        try:
            u = st.target(j)
            assert np.float64(u) * np.float64(st.pot) == st.running_sum(j)
        except kr.Inexact:
            refused += 1
    assert 0 < refused < 1000                          # bell-shaped data: fl(fl(rs / pot) * pot) is rs for most samples, not for all
    x, mean = kr.exact_data(3000, 5, 9, 0)
    st = kr.Stepper((x - mean).astype(np.float32), 3, 0.4)
    with pytest.raises(kr.Inexact):                     # the total itself would need u = 1
        st.target(st.positive_from(2999, -1))
    with pytest.raises(kr.Inexact):                     # a sample without an increment of its own
        st.target(int(np.nonzero(st.closest == 0)[0][0]))


@pytest.mark.parametrize("name", ALL)
def test_case_is_the_oracle_and_its_targets_land(name):
    """build() itself asserts that the round-by-round replay gives oracle.kmeans_plusplus's indices from the same draws, that the
    draws are consumed exactly and (exact cases) the exactness precondition; here: every aimed draw landed on the sample it names."""
    b = kr.build(name)
    assert b.ids.shape == (b.case.k,) and b.ids[0] == b.first_id
    aimed = 0
    for rd in b.stepper.rounds:
        for t, want in enumerate(rd["wants"]):
            if want is not None:
                assert rd["cand"][t] == want, (name, rd["tags"][t], rd["cand"][t], want)
                aimed += 1
        assert all((not bf) or gf for bf, gf in zip(rd["block_fb"], rd["group_fb"]))     # see the inventory below
    print(f"{name}: {len(b.stepper.rounds)} rounds of {b.stepper.T}, {aimed} aimed draws")


def test_inventory_of_the_edges_reached():
    tags, fb = {}, {"group": 0, "block": 0, "sample": 0, "sample_alone": 0}
    pot0 = potinf = rnan = ties = t8 = 0
    for b, rd in _rounds(ALL):
        for t, tag in enumerate(rd["tags"]):
            tags[tag] = tags.get(tag, 0) + 1
            fb["group"] += rd["group_fb"][t]
            fb["block"] += rd["block_fb"][t]
            fb["sample"] += rd["sample_fb"][t]
            fb["sample_alone"] += rd["sample_fb"][t] and not rd["block_fb"][t]
        pot0 += rd["pot"] == 0
        potinf += bool(np.isinf(rd["pot"]))
        rnan += bool(np.isnan(rd["r"]).any())
        p, c = rd["pots"], rd["cand"]
        ties += any(p[t] == p[0] and c[t] != c[0] and p[0] == p.min() for t in range(1, len(c)))
        t8 += len(c) == kr.PP_TMAX
    print("draws by tag:", dict(sorted(tags.items())))
    print("fallbacks:", fb, "rounds with potential 0:", pot0, "inf:", potinf, "NaN r:", rnan, "winner ties:", ties, "rounds of 8:", t8)
    assert TARGET_TAGS <= set(tags), sorted(TARGET_TAGS - set(tags))
    # The group fallback: no running group total reaches r (r > G[-1], inf or NaN).  The block fallback is only ever taken below it:
    # a group's total is G[g] + (W[last] + S[last]), the very sum the block search compares with, so a group that reaches r has
    # a block that does (asserted per case above).  The sample fallback is taken alone as well: the block's butterfly sum reaches r,
    # its left-to-right sum does not.
    assert fb["group"] > 0 and fb["block"] > 0 and fb["sample"] > 0 and fb["sample_alone"] > 0, fb
    assert pot0 > 0 and potinf > 0 and rnan > 0 and ties > 0 and t8 > 300
    # u = 1 - 2^-53 on a float32 potential that rounded up: r > total
    assert any(rd["tags"][t] == "u_max" and rd["group_fb"][t] and np.isfinite(rd["r"][t]) for _, rd in _rounds(SMALL) for t in range(len(rd["tags"])))
    b = kr.build("tiny-1e-20-n2000-k4")
    d = orc._pp_dist(b.xc[b.first_id], b.xc)
    pos = d[d > 0]
    print("scale 1e-20:", int((pos < kr.F32_TINY).sum()), "of", pos.size, "positive distances are subnormal")
    assert (pos < kr.F32_TINY).sum() > pos.size / 2


@pytest.mark.parametrize("name", [c.name for c in kr.CASES if c.exact or c.family == "degenerate"])
def test_scikit_learn_itself_gives_the_oracles_indices(name):
    """On exact data (and where every potential is 0 or inf) a float32 sum is the same in any order, so scikit-learn's
    _kmeans_plusplus, fed the scripted draws, must give the oracle's indices index for index."""
    pytest.importorskip("sklearn")
    from sklearn.cluster._kmeans import _kmeans_plusplus

    b = kr.build(name)
    if not kr.sklearn_comparable(b):
        assert not b.case.exact
        return                                          # oracle-only: finite inexact potentials (the tiny scale, the offset vector)
    xc = b.xc if b.xc is not None else (b.x - b.x_mean).astype(np.float32)
    X = xc.reshape(-1, 1)
    draws = kr.ScriptedDraws(b.first_u, b.uniforms)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        centers, ids = _kmeans_plusplus(X, b.case.k, (X * X).sum(axis=1), np.ones(b.case.n, dtype=np.float32), draws)
    draws.assert_consumed()
    assert np.array_equal(ids, b.ids), (name, int((ids != b.ids).sum()))
    assert np.array_equal(centers.ravel(), xc[b.ids])


def test_degenerate_cases_compared_with_scikit_learn():
    """Which of the inexact cases the comparison above covers: the huge scale (every potential inf); not the tiny scale and the offset
    vectors (finite potentials that depend on the order of a float32 sum)."""
    got = {c.name: kr.sklearn_comparable(kr.build(c.name)) for c in kr.CASES if c.family == "degenerate"}
    assert got == {"constant-n2000-k4": True, "three-values-n1500-k5": True, "tiny-1e-20-n2000-k4": False, "huge-1e18-n2000-k4": True,
                   "offset-n5000-k6-own-mean": False, "offset-n5000-k6-given-mean": False}, got
    b = kr.build("huge-1e18-n2000-k4")
    assert b.ids.tolist() == [b.first_id] + [b.case.n - 1] * 3
    b = kr.build("constant-n2000-k4")
    assert b.ids.tolist() == [b.first_id, 0, 0, 0]
    b = kr.build("three-values-n1500-k5")
    assert len(set(b.xc[b.ids[:3]].tolist())) == 3 and b.ids[3:].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ the host half of the ABI
@pytest.fixture(scope="module")
def lib():
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import build as nbuild

    nbuild.build_native()
    return nat.load()


def test_trial_count(lib):
    assert kr.NNC_KMAX == 1040
    for k in range(1, kr.NNC_KMAX + 1):
        assert lib.nnc_kmeanspp_trials(k) == 2 + int(np.log(k)), k
    assert [lib.nnc_kmeanspp_trials(k) for k in (0, -1, -(2 ** 31))] == [0, 0, 0]
    assert lib.nnc_kmeanspp_trials(403) == 7 and lib.nnc_kmeanspp_trials(404) == 8 == kr.PP_TMAX == lib.nnc_kmeanspp_trials(kr.NNC_KMAX)


def test_workspace_size(lib):
    for n in (1, 2, 255, 1023, 1024, 1025, 262_143, 262_144, 262_145, 524_289, kr.N_65_GROUPS, kr.N_66_GROUPS, 25_000_000, 2 ** 29 - 1):
        for k in (1, 2, 404, kr.NNC_KMAX):
            got = lib.nnc_kmeanspp_workspace_bytes(n, k)
            assert got == kr.workspace_bytes(n, k) and got % 256 == 0, (n, k, got)
    assert [lib.nnc_kmeanspp_workspace_bytes(n, k) for n, k in ((0, 4), (-1, 4), (100, 0), (100, -3))] == [0, 0, 0, 0]


def test_argument_errors_come_before_any_device_call(lib):
    """Every pointer here is a made-up address: a call that got as far as a launch would not return an argument error."""
    n, k = 5000, 16
    wsb = lib.nnc_kmeanspp_workspace_bytes(n, k)
    X, U, S, I, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000

    def call(x=X, n=n, k=k, first=7, u=U, s=S, i=I, ws=WS, wsb=wsb):
        return lib.nnc_kmeanspp_seed_f32(x, n, ctypes.c_float(0.0), k, first, u, s, i, ws, wsb, None)

    for what, kw in {"n = 0": dict(n=0), "n < 0": dict(n=-4), "k = 0": dict(k=0), "k < 0": dict(k=-1), "k > NNC_KMAX": dict(k=kr.NNC_KMAX + 1),
                     "first_id < 0": dict(first=-1), "first_id = n": dict(first=n), "first_id > n": dict(first=n + 9), "no x": dict(x=None),
                     "no seeds_out": dict(s=None), "no seed_ids_out": dict(i=None), "no uniforms, k > 1": dict(u=None), "no workspace": dict(ws=None),
                     "workspace not 256-byte aligned": dict(ws=WS + 128), "workspace 4 bytes off": dict(ws=WS + 4)}.items():
        assert call(**kw) == NNC_EINVAL, what
    for short in (0, 1, wsb - 256, wsb - 1):
        assert call(wsb=short) == NNC_ENOSPACE, short
    assert call(ws=WS + 4, wsb=wsb - 1) == NNC_ENOSPACE      # the size is looked at first
    assert call(k=kr.NNC_KMAX, wsb=lib.nnc_kmeanspp_workspace_bytes(n, kr.NNC_KMAX) - 1) == NNC_ENOSPACE
