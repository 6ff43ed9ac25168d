"""Weight tensors a trained network actually has, where ``synth.weights`` only gives a zero-mean bell: heavy tails, a few extreme
values, a mean far from zero, one sign only, an empty middle, three values.  What depends on the DATA rather than the shape (the cell
grid of the E-step, the width of the sort keys, the 31-bin histogram behind the density init, the fixed-point shift, the prune
threshold) is exercised by these and by nothing else in the suite.

Every recipe is float64 ``+ * abs where round`` on ``synth.irwin_hall12`` variates (exactly representable, integer-made) followed by
one correctly rounded cast to float32: no libm, so the tensors are bit-identical wherever they are rebuilt.  The goldens
(tests/golden/ref_shapes.*, made by tests/golden/make_goldens_shapes.py from the reference itself) store each input's SHA-256 and
every test that rebuilds an input checks it.  Test infrastructure only."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from neural_network_compression_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(os.path.dirname(HERE), "golden")


def _cubic(z, u, n):
    return (0.02 * z * z * z).astype(np.float32)


def _quintic(z, u, n):
    return (0.004 * z * z * z * z * z).astype(np.float32)


def _outliers(z, u, n):
    w = (0.05 * z).astype(np.float32)
    w[:: max(1, n // 7)] *= np.float32(400)
    return w


def _gain(z, u, n):
    return (1.0 + 0.02 * z).astype(np.float32)


def _onesided(z, u, n):
    return np.abs(0.05 * z).astype(np.float32)


def _negative(z, u, n):
    return (-1.0 * np.abs(0.05 * z)).astype(np.float32)


def _skew(z, u, n):
    return (0.05 * (z + 0.35 * z * z)).astype(np.float32)


def _bimodal(z, u, n):
    return (0.05 * z + np.where(u > 0, 0.4, -0.3)).astype(np.float32)


def _ternary(z, u, n):
    r = np.round(z)
    return np.where(r > 0, 0.125, np.where(r < 0, -0.125, 0.0)).astype(np.float32)


# name -> (recipe, seed of z; u comes from seed + 1)
RECIPES = {
    "cubic": (_cubic, 12000), "quintic": (_quintic, 12002), "outliers": (_outliers, 12004), "gain": (_gain, 12006),
    "onesided": (_onesided, 12008), "negative": (_negative, 12010), "skew": (_skew, 12012), "bimodal": (_bimodal, 12014),
    "ternary": (_ternary, 12016),
}
SHAPES = tuple(RECIPES)

# the pruned input with fewer non-zero weights than centres: the eight spikes of `outliers` at n = 3000 put sigma at about 1, five
# times the largest bulk weight, so q = 1 leaves the spikes above sigma alone -- fewer than the 16 / 17 centres of 4 bits
FEWER_NONZERO_THAN_CENTRES = ("outliers", 3000, 1.0)
NEARLY_ALL_PRUNED = ("outliers", 50_000, 1.0)


def make(name: str, n: int) -> np.ndarray:
    """The unpruned float32 vector of n weights of the named recipe."""
    fn, seed = RECIPES[name]
    z = synth.irwin_hall12(n, seed)
    u = synth.irwin_hall12(n, seed + 1)
    return np.ascontiguousarray(fn(z, u, n))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def qtag(q) -> str:
    return "qnone" if q is None else f"q{q:g}"


def input_key(name, n, q) -> str:
    return f"{name}/n{n}/{qtag(q)}"


# ------------------------------------------------------------------ the matrix of golden fits
NS = (3000, 6000, 50_000)                     # the one-launch reference-arithmetic form (<= 4096), just above it, mid-sized
QS = (None, 1.0)
MODES = (("linear", 4), ("density", 4), ("density", 5), ("linear", 2))
MAX_REF_ITER = 150                            # fits the reference needs more iterations for are left out of the goldens


def fit_key(name, n, q, mode, bits, extra="") -> str:
    return f"fit/{input_key(name, n, q)}/{mode}{bits}{extra}"


def matrix():
    """(key, name, n, q, mode, bits, forgy_seed, max_iter) of every fit the golden script runs the reference on."""
    out = []
    for name in SHAPES:
        for n in NS:
            for q in QS:
                for mode, bits in MODES:
                    out.append((fit_key(name, n, q, mode, bits), name, n, q, mode, bits, None, None))
    for name in ("outliers", "cubic"):        # K = 129 / 257: the launch-per-iteration form, 16-bit indices
        for bits in (7, 8):
            out.append((fit_key(name, 50_000, None, "density", bits), name, 50_000, None, "density", bits, None, None))
    out.append((fit_key("gain", 50_000, None, "forgy", 5), "gain", 50_000, None, "forgy", 5, 501, None))
    out.append((fit_key("outliers", 6000, None, "forgy", 5), "outliers", 6000, None, "forgy", 5, 502, None))
    out.append((fit_key("bimodal", 235_200, None, "linear", 4), "bimodal", 235_200, None, "linear", 4, None, None))
    out.append((fit_key("outliers", 235_200, None, "linear", 4), "outliers", 235_200, None, "linear", 4, None, None))
    out.append((fit_key("cubic", 50_000, None, "density", 5, "/maxiter20"), "cubic", 50_000, None, "density", 5, None, 20))
    return out


# ------------------------------------------------------------------ the goldens
class ShapeGoldens:
    def __init__(self):
        with open(os.path.join(GOLDEN_DIR, "ref_shapes.json")) as f:
            self.manifest = json.load(f)
        self.arrays = dict(np.load(os.path.join(GOLDEN_DIR, "ref_shapes.npz")))
        self.inputs = self.manifest["inputs"]
        self.cases = self.manifest["cases"]
        self.dropped = self.manifest["dropped"]
        for key, name, n, q, mode, bits, forgy_seed, max_iter in matrix():     # what the key says, spelt out
            if key in self.cases:
                self.cases[key].update(shape=name, n=n, q=q, mode=mode, bits=bits, forgy_seed=forgy_seed, max_iter=max_iter)
            self.inputs[input_key(name, n, q)].update(shape=name, n=n, q=q)

    def init(self, c):
        return self.arrays["init"][c["off"]: c["off"] + c["K"]]

    def centers(self, c):
        return self.arrays["centers"][c["off"]: c["off"] + c["K"]]

    def bincount(self, c):
        return self.arrays["bincount"][c["off"]: c["off"] + c["K"]].astype(np.int64)

    def cdfs(self, i):
        """(xnew, cdf) the reference computed on the non-zero weights of input entry i."""
        return self.arrays["xnew"][i["row"]], self.arrays["cdf"][i["row"]]

    def input_of(self, c):
        return self.inputs[input_key(c["shape"], c["n"], c["q"])]

    def messages(self, c, field="warnings"):
        return [tuple(self.manifest["messages"][j]) for j in c.get(field, [])]

    def fits(self):
        """Keys of the fits the reference completed (it raises on none of the matrix; a case may still carry warnings)."""
        return sorted(k for k, c in self.cases.items() if "n_iter" in c)


_G = None


def goldens() -> ShapeGoldens:
    global _G
    if _G is None:
        _G = ShapeGoldens()
    return _G


_INPUTS: dict = {}


def pruned_input(name, n, q):
    """(w, mask): the tensor a golden fit was made on -- pruned in place as the reference prunes it (oracle.prune_weigth, pinned to
    the reference's masks by tests/test_oracle_shapes.py) -- and the mask (None without pruning).  Cached; callers copy before writing."""
    from oracle import oracle as orc

    k = (name, n, q)
    if k not in _INPUTS:
        w = make(name, n)
        mask = orc.prune_weigth(w, q, True) if q is not None else None
        w.setflags(write=False)
        _INPUTS[k] = (w, mask)
    return _INPUTS[k]


def case_input(c):
    return pruned_input(c["shape"], c["n"], c["q"])[0]


def case_cdfs(g: ShapeGoldens, c):
    return g.cdfs(g.input_of(c))


# ------------------------------------------------------------------ categories of the oracle's A <-> B gap
def category(c) -> str:
    """tight / summation / divergent from the CPU-computed gap stored with the case (tests/helpers/ab_gap.py's two ceilings)."""
    from tests.helpers import ab_gap

    g = c["gap"]
    if g["n_iter"] == c["n_iter"]:
        if g["err"] <= ab_gap.NORTH_STAR_TOL and g["hist_l1"] == 0:
            return "tight"
        if g["err"] <= ab_gap.SUMMATION_ERROR_CEILING:
            return "summation"
    return "divergent"


RULE = "rule"      # the relocation of empty clusters: which far sample goes to which of several empty clusters is the order numpy.argpartition
#                    leaves (the device: descending distance), and so is the choice between two different values equally far at the cut
SUMS = "sums"      # scikit-learn's float32 running sums against exact sums: a boundary sample changes sides, or another sample is the
#                    farthest at the next event, and the trajectories part
BOTH = "both"      # either difference alone already parts them


def cause(c) -> str:
    """Why a divergent fit diverges, from the two single-difference oracle fits recorded with it (make_goldens_shapes.py: the
    reference's sums with the device's relocation rule; the device's sums with numpy.argpartition's own selection)."""
    why = c["why"]
    return BOTH if (why["rule"] and why["sums"]) else RULE if why["rule"] else SUMS


# Golden fits (ternary aside: three values, every relocation a tie) on which the oracle in the device's arithmetic does not end where
# the reference ended, each with its cause: 16 of 201.  From the CPU run of tests/golden/make_goldens_shapes.py;
# tests/test_oracle_shapes.py checks that this is exactly the set the stored gaps give and that each cause is what the recorded
# single-difference fits give.  Their A <-> B gap is recorded in the manifest and not bounded.  None of them has a tie between two
# DIFFERENT values at a cut (the ties the oracle counts on them are between equal values: the zeros of a pruned tensor).
DIVERGENT = {
    "fit/bimodal/n50000/q1/density4": SUMS, "fit/bimodal/n50000/q1/density5": SUMS, "fit/bimodal/n6000/q1/density4": SUMS,
    "fit/outliers/n3000/q1/density4": RULE, "fit/outliers/n3000/q1/density5": RULE, "fit/outliers/n3000/q1/linear4": RULE,
    "fit/outliers/n50000/q1/density4": BOTH, "fit/outliers/n50000/q1/density5": BOTH, "fit/outliers/n50000/q1/linear4": BOTH,
    "fit/outliers/n6000/q1/density4": BOTH,
    "fit/cubic/n50000/qnone/density8": RULE, "fit/outliers/n50000/qnone/density7": SUMS,
    "fit/outliers/n50000/qnone/density8": BOTH, "fit/outliers/n6000/qnone/linear4": SUMS,
    "fit/skew/n50000/q1/density4": SUMS,
    "fit/skew/n50000/qnone/linear4": SUMS,     # no relocation at all: 135 iterations there, 136 here; centres 5.5e-4 apart, just above the ceiling
}
DIVERGENT_CAP = 0.1         # at most one golden fit in ten, ternary aside
