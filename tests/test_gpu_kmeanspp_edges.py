"""k-means++ seeding on the device at its edges (run with -m gpu on an MI355X): nnc_kmeanspp_seed_f32 through the raw ABI on the
scripted cases of tests/helpers/kmeanspp_ref.py -- draws placed exactly on running-sum values, on plateaus of zero increments that
span block and group boundaries, past the total, on potentials of 0 and inf, on candidates of equal potential, with all eight
trial slots, on more than 64 groups -- and the whole mode="kmeans++" on the heavy-tailed, offset and few-valued tensors of
tests/helpers/shapes.py.

Expected in every case: the ids of oracle.kmeans_plusplus fed the same scripted draws, in all k positions, and
seeds == float32(x[ids] - x_mean) bit for bit.  On the exact cases tests/test_kmeanspp_ref.py holds the oracle to scikit-learn's own
_kmeans_plusplus index for index, so the device is pinned to scikit-learn itself there.  Every buffer is the test's own: outputs
and workspace (exactly the queried size) inside sentinel frames that must come back untouched, x a slice of a longer buffer of NaN
(once 16-byte aligned, once one element further), and a second call must give the same bits."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests.helpers import kmeanspp_ref as kr  # noqa: E402
from tests.helpers import shapes  # noqa: E402

GUARD = 64
F32_SENTINEL = 0x4B1D4B1D
I64_SENTINEL = -0x0123456789ABCDEF
WS_BYTE = 0xA5


@pytest.fixture(scope="module")
def nnc():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from neural_network_compression_amd import _native, kmeans
    from neural_network_compression_amd.common import utility

    class NS:
        pass

    ns = NS()
    ns.L = _native.load()   # fails loudly if the HIP library is missing
    ns.nat, ns.kmeans, ns.utility = _native, kmeans, utility
    return ns


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def seed_raw(nnc, x, x_mean, k, first_id, uniforms, x_off):
    """One call of nnc_kmeanspp_seed_f32 with buffers made here; returns (seeds, ids) after checking every frame."""
    L = nnc.L
    n = x.size
    xbuf = torch.full((x_off + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    xbuf[x_off: x_off + n] = torch.from_numpy(x)
    xt = xbuf[x_off: x_off + n]
    assert xt.data_ptr() % 16 == (0 if x_off % 4 == 0 else 4 * (x_off % 4))
    uni = torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).cuda() if k > 1 else None
    seeds = torch.full((GUARD + k + GUARD,), F32_SENTINEL, dtype=torch.int32, device="cuda")
    ids = torch.full((GUARD + k + GUARD,), I64_SENTINEL, dtype=torch.int64, device="cuda")
    wsb = int(L.nnc_kmeanspp_workspace_bytes(n, k))
    assert wsb == kr.workspace_bytes(n, k)
    wbuf = torch.full((wsb + 1024,), WS_BYTE, dtype=torch.uint8, device="cuda")
    lo = 256 + (-(wbuf.data_ptr() + 256)) % 256
    ws_ptr = wbuf.data_ptr() + lo
    assert ws_ptr % 256 == 0 and 256 <= lo < 512
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.nnc_kmeanspp_seed_f32(xt.data_ptr(), n, ctypes.c_float(float(x_mean)), k, int(first_id), 0 if uni is None else uni.data_ptr(),
                                 seeds[GUARD:].data_ptr(), ids[GUARD:].data_ptr(), ws_ptr, wsb, stream)
    nnc.nat.check(rc)
    torch.cuda.synchronize()
    sh, ih = seeds.cpu().numpy(), ids.cpu().numpy()
    assert np.all(sh[:GUARD] == F32_SENTINEL) and np.all(sh[GUARD + k:] == F32_SENTINEL), "seeds_out frame"
    assert np.all(ih[:GUARD] == I64_SENTINEL) and np.all(ih[GUARD + k:] == I64_SENTINEL), "seed_ids_out frame"
    assert bool((wbuf[:lo] == WS_BYTE).all().item()) and bool((wbuf[lo + wsb:] == WS_BYTE).all().item()), "workspace frame"
    assert bool(torch.isnan(xbuf[:x_off]).all().item()) and bool(torch.isnan(xbuf[x_off + n:]).all().item())
    assert np.all(ih[GUARD: GUARD + k] != I64_SENTINEL), "an id was not written"
    return sh[GUARD: GUARD + k].view(np.float32).copy(), ih[GUARD: GUARD + k].copy()


def check_case(nnc, name, offsets=(4, 5)):
    b = kr.build(name)
    c = b.case
    want_seeds = (b.x[b.ids] - b.x_mean).astype(np.float32)
    runs = []
    for x_off in offsets:
        for rep in range(2 if x_off == offsets[0] else 1):
            runs.append(seed_raw(nnc, b.x, b.x_mean, c.k, b.first_id, b.uniforms, x_off))
    for seeds, ids in runs:
        assert np.array_equal(ids, b.ids), (name, int((ids != b.ids).sum()), np.nonzero(ids != b.ids)[0][:4], ids[ids != b.ids][:4], b.ids[ids != b.ids][:4])
        assert np.array_equal(_u32(seeds), _u32(want_seeds)), name
        assert np.array_equal(_u32(seeds), _u32(runs[0][0])) and np.array_equal(ids, runs[0][1])
    return b


def _names(family):
    return [c.name for c in kr.CASES if c.family == family]


@pytest.mark.parametrize("name", _names("geometry"))
def test_block_and_group_geometry(nnc, name):
    check_case(nnc, name)


@pytest.mark.parametrize("name", _names("groups"))
def test_more_than_64_groups(nnc, name):
    """The second step of the group loop: 65 groups (the last with two blocks, the last block with one sample), draws at group 0,
    at the group 63 / 64 boundary and into group 64; and 66 groups, where a draw into group 64 is not what the fallback gives."""
    check_case(nnc, name, offsets=(4,) if name.startswith("groups66") else (5,))


@pytest.mark.parametrize("name", _names("trials"))
def test_all_eight_trial_slots(nnc, name):
    b = check_case(nnc, name)
    assert b.stepper.T == (7 if b.case.k == 403 else 8)


@pytest.mark.parametrize("name", _names("plateau"))
def test_draws_on_below_and_above_a_plateau(nnc, name):
    check_case(nnc, name)


@pytest.mark.parametrize("name", _names("degenerate"))
def test_degenerate_potentials(nnc, name):
    b = kr.build(name)
    if b.case.stats_mean:          # x_mean as the layer call computes it
        st = nnc.kmeans.LayerStats(torch.from_numpy(b.x).cuda())
        assert shapes.f32_bits(st.mean) == shapes.f32_bits(b.x_mean)
    if b.case.x_mean is not None:  # ... and one that is not the mean: the ABI takes it as given
        assert shapes.f32_bits(b.x_mean) != shapes.f32_bits(orc.np_mean(b.x))
    check_case(nnc, name)


@pytest.mark.parametrize("name", _names("ties"))
def test_first_of_equal_potentials_wins(nnc, name):
    b = check_case(nnc, name)
    tied = [rd for rd in b.stepper.rounds
            if any(rd["pots"][t] == rd["pots"][rd["winner"]] and rd["cand"][t] != rd["cand"][rd["winner"]] for t in range(rd["winner"] + 1, b.stepper.T))]
    assert tied, "no round in which a later slot holds another candidate of the winning potential"


# ------------------------------------------------------------------------------------------ the whole mode on the hard distributions
MODE_CASES = [(name, n, q, nbits) for name in shapes.SHAPES for n in (3000, 6000) for q in shapes.QS for nbits in (2, 5)]
MODE_CASES += [(shapes.NEARLY_ALL_PRUNED[0], shapes.NEARLY_ALL_PRUNED[1], q, nbits) for q in shapes.QS for nbits in (2, 5)]
_RELOCATED: dict = {}


def _summary(o):
    i = o.reloc_info_
    return tuple(int(i.get(f, 0)) for f in ("reloc_events", "reloc_multi", "reloc_ties_distinct", "reloc_ties"))


def fit_mode(nnc, name, n, q, nbits):
    key = (name, n, q, nbits)
    if key in _RELOCATED:
        return _RELOCATED[key]
    w = shapes.pruned_input(name, n, q)[0]
    K = 2 ** nbits
    seed = 40 + len(name) + nbits + n % 7
    np.random.seed(seed)
    ob = orc.kmeans_plusplus_fit(w.copy().ravel(), K, accum="device")
    nxt_o = np.random.rand()
    np.random.seed(seed)
    qw, km = nnc.utility.get_quantized_weight(w.copy(), bits=nbits, mode="kmeans++")
    nxt_d = np.random.rand()
    assert nxt_d == nxt_o, key
    assert km.n_iter_ == ob.n_iter_, (key, km.n_iter_, ob.n_iter_)
    assert np.array_equal(_u32(km.cluster_centers_.ravel()), _u32(ob.cluster_centers_.ravel())), key
    assert np.array_equal(km.labels_, ob.labels_), (key, int((km.labels_ != ob.labels_).sum()))
    assert np.array_equal(_u32(qw.ravel()), _u32(ob.cluster_centers_.ravel()[ob.labels_])), key
    events, multi, distinct, any_tie = _summary(ob)
    print(f"{key}: n_iter {km.n_iter_}; events {km.n_relocations_}/{events}, multi {km.n_reloc_multi_}/{multi}, tie {km.reloc_tie_}/{distinct} of {any_tie}")
    assert km.n_relocations_ == events and km.n_reloc_multi_ == multi, (key, km.n_relocations_, events, km.n_reloc_multi_, multi)
    # a relocation tie between two different values: reported, and the fit still the oracle's bit for bit (as tests/test_gpu_shapes.py)
    assert (km.reloc_tie_ != 0) == (distinct != 0), (key, km.reloc_tie_, distinct, any_tie)
    assert km.reloc_tie_ <= any_tie, (key, km.reloc_tie_, any_tie)
    assert km.arith_ == ("reference" if orc.device_arith(n, K)[0] == "A" else "fixed"), key
    _RELOCATED[key] = events
    return events


@pytest.mark.parametrize("name,n,q,nbits", MODE_CASES)
def test_whole_mode_on_the_hard_distributions(nnc, name, n, q, nbits):
    """n_iter_, centres, labels, the next random number and the relocation counts, all against the oracle's fit from the same draws.
    Among them: fits from duplicate seeds whose first iteration finds empty clusters while every sample sits on a seed -- all
    distances 0, scikit-learn relocates nothing, and neither the oracle nor the device counts a relocation (nnc_kmeans_status.n_reloc_null)."""
    fit_mode(nnc, name, n, q, nbits)


def test_few_valued_inputs_relocate(nnc):
    """Few-valued inputs give duplicate seeds (the potential reaches 0, every later seed is sample 0), so the first Lloyd iteration
    meets empty clusters."""
    events = [fit_mode(nnc, name, n, q, 5) for name, n, q in (("ternary", 3000, None), ("ternary", 6000, None), (*shapes.NEARLY_ALL_PRUNED[:2], 1.0))]
    assert all(e > 0 for e in events), events
