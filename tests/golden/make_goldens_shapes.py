#!/usr/bin/env python3
"""Golden vectors of the reference on heavy-tailed, offset and few-valued weights (tests/helpers/shapes.py).

Runs ONLY in the build container, like make_goldens.py, whose ``load_reference`` it reuses: the reference's own

    prune_weigth, get_weight_distribution, get_quantized_weight      (neural_network_compression/common/utility.py)

on one thread, on every input of ``shapes.matrix()``.  Per input: SHA-256 of the tensor, sigma, mask, the 300-point weight
distribution of the non-zero weights.  Per fit: the init the reference handed to KMeans, n_iter_, centres, index histogram, SHA-256 of
the indices, the warnings scikit-learn raised (or the exception, where the reference raises), the oracle's relocation summary in the
reference's arithmetic (mode A) and in the device's, the CPU-computed gap between the two (what tests/helpers/ab_gap.gap
computes for the older goldens) and, where that gap is a divergence, which of the two differences brings it about.  Fits the reference needs more than shapes.MAX_REF_ITER iterations for are dropped.

Output: tests/golden/ref_shapes.npz (arrays) + tests/golden/ref_shapes.json (manifest); rerunning reproduces both byte for byte.
"""
from __future__ import annotations

import json
import os
import sys
import warnings
import zipfile

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import sklearn  # noqa: E402
from threadpoolctl import threadpool_limits  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402
from tests.golden.make_goldens import load_reference, strip_zeros  # noqa: E402
from tests.helpers import ab_gap, shapes  # noqa: E402

# Arrays are packed (a zip member per small array costs more than the array): the K-sized vectors of all fits end to end in
# init / centers / bincount (a case stores its offset), the 300-point distributions as rows of xnew / cdf (an input stores its row).
PACK = {"init": [], "centers": [], "bincount": [], "xnew": [], "cdf": []}
MAN = {"versions": {"numpy": np.__version__, "sklearn": sklearn.__version__}, "dtypes": {}, "messages": [], "inputs": {}, "cases": {}, "dropped": {}}
MAX_ITER = [None]
OFF = [0]


def dtype_is(name, a):
    assert MAN["dtypes"].setdefault(name, str(np.asarray(a).dtype)) == str(np.asarray(a).dtype), name


def caught(ws):
    """Indices into MAN["messages"] ([category, text]) of the warnings raised."""
    out = []
    for w in ws:
        m = [type(w.message).__name__, str(w.message)]
        if m not in MAN["messages"]:
            MAN["messages"].append(m)
        out.append(MAN["messages"].index(m))
    return out


def gen_input(ref, name, n, q):
    ikey = shapes.input_key(name, n, q)
    if ikey in MAN["inputs"]:
        return
    w = shapes.make(name, n)
    e = {"input_sha256": shapes.sha(w),
         "mean_bits": shapes.f32_bits(np.mean(w)), "var_bits": shapes.f32_bits(np.var(w)), "sigma_bits": shapes.f32_bits(np.std(w)),
         "min_bits": shapes.f32_bits(w.min()), "max_bits": shapes.f32_bits(w.max())}
    if q is not None:
        mask = ref.prune_weigth(w, threshold=q, std_smooth=True)
        e.update({"mask_sha256": shapes.sha(np.packbits(mask.ravel())), "nzeroed": int(mask.sum())})
    nz = strip_zeros(w)
    e["n_nonzero"] = int(nz.size)
    try:
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            xnew, cdf = ref.get_weight_distribution(nz)
        if ws:
            e["cdf_warnings"] = caught(ws)
        dtype_is("xnew", xnew), dtype_is("cdf", cdf)
        e["row"] = len(PACK["xnew"])
        PACK["xnew"].append(np.asarray(xnew))
        PACK["cdf"].append(np.asarray(cdf))
        e["cdf_distinct"] = int(np.unique(np.asarray(cdf)).size)
    except Exception as ex:  # noqa: BLE001  (the reference's own failure is the recorded outcome)
        e["cdf_raises"] = {"type": type(ex).__name__, "message": str(ex)}
    MAN["inputs"][ikey] = e


def reference_input(ref, name, n, q):
    w = shapes.make(name, n)
    if q is not None:
        ref.prune_weigth(w, threshold=q, std_smooth=True)
    return w


def gen_fit(ref, captured, key, name, n, q, mode, bits, forgy_seed, max_iter):
    w = reference_input(ref, name, n, q)
    ikey = shapes.input_key(name, n, q)
    entry = {}
    cdfs = None
    if mode == "density":
        i = MAN["inputs"][ikey]
        if "cdf_raises" in i:
            entry["raises"] = i["cdf_raises"]
            MAN["cases"][key] = entry
            return
        cdfs = (PACK["xnew"][i["row"]], PACK["cdf"][i["row"]])
    if forgy_seed is not None:
        np.random.seed(forgy_seed)
    captured.pop("init", None)
    MAX_ITER[0] = max_iter
    try:
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            qw, km = ref.get_quantized_weight(w.copy(), bits=bits, mode=mode, cdfs=cdfs)
    except Exception as ex:  # noqa: BLE001
        entry["raises"] = {"type": type(ex).__name__, "message": str(ex)}
        MAN["cases"][key] = entry
        return
    finally:
        MAX_ITER[0] = None
    if ws:
        entry["warnings"] = caught(ws)
    if km is None:
        entry["passthrough"] = True
        MAN["cases"][key] = entry
        return
    if max_iter is None and km.n_iter_ > shapes.MAX_REF_ITER:
        MAN["dropped"][key] = int(km.n_iter_)
        return
    centers = km.cluster_centers_.ravel()
    labels = km.labels_
    init = captured["init"].ravel().astype(np.float32)
    K = int(centers.size)
    kw = {} if max_iter is None else {"max_iter": max_iter}
    oa = orc.kmeans_lloyd(w.ravel(), init, accum="A", **kw)
    od = orc.kmeans_lloyd(w.ravel(), init, accum="device", **kw)
    a_equal = (oa.n_iter_ == km.n_iter_ and np.array_equal(oa.cluster_centers_.ravel(), centers) and np.array_equal(oa.labels_, labels))
    if not a_equal:
        print("oracle mode A differs from the reference:", key, oa.n_iter_, km.n_iter_, flush=True)
    bc = np.bincount(labels, minlength=K).astype(np.int64)
    bd = np.bincount(od.labels_, minlength=K).astype(np.int64)
    entry.update({
        "K": K, "off": OFF[0], "n_iter": int(km.n_iter_), "init_distinct": int(np.unique(init).size),
        "labels_sha256": shapes.sha(labels.astype(np.int32)),
        "reloc_A": {k: int(v) for k, v in sorted(oa.reloc_info_.items())},
        "reloc_dev": {k: int(v) for k, v in sorted(od.reloc_info_.items())},
        "gap": {"n_iter": int(od.n_iter_), "err": ab_gap.centre_err(od.cluster_centers_, centers), "hist_l1": int(np.abs(bd - bc).sum()),
                "labels_differing": int((od.labels_ != labels).sum()), "arith": orc.device_arith(n, K)[0]},
    })
    if shapes.category(entry) == "divergent":
        # which of the two differences to the reference does it: the device's relocation rule with the reference's sums, or the
        # device's sums with numpy.argpartition's own selection (each fit sorted as the gap itself is)
        acc = orc.device_arith(n, K)[0]
        why = {}
        for name_, fit in (("rule", orc.kmeans_lloyd(w.ravel(), init, accum="A", reloc="descending", **kw)),
                           ("sums", orc.kmeans_lloyd(w.ravel(), init, accum=acc, reloc="argpartition", **kw))):
            bf = np.bincount(fit.labels_, minlength=K).astype(np.int64)
            why[name_] = shapes.category({"n_iter": int(km.n_iter_), "gap": {"n_iter": int(fit.n_iter_), "err": ab_gap.centre_err(fit.cluster_centers_, centers),
                                                                             "hist_l1": int(np.abs(bf - bc).sum())}}) == "divergent"
        entry["why"] = why
    dtype_is("init_as_given", captured["init"]), dtype_is("centers", centers), dtype_is("labels", labels), dtype_is("quantized", qw)
    assert np.array_equal(qw, centers[labels].reshape(qw.shape))       # (so the decoded tensor needs no hash of its own)
    PACK["init"].append(init), PACK["centers"].append(centers), PACK["bincount"].append(bc.astype(np.int32))
    OFF[0] += K
    MAN["cases"][key] = entry


def save_npz(path, arrays):
    """np.savez_compressed with fixed member times, so that a rerun reproduces the file byte for byte."""
    import io

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[name], allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


def main():
    ref, captured = load_reference()
    inner = ref.KMeans

    def kmeans_with_cap(*args, **kwargs):
        if MAX_ITER[0] is not None:
            kwargs["max_iter"] = MAX_ITER[0]
        return inner(*args, **kwargs)

    ref.KMeans = kmeans_with_cap
    with threadpool_limits(1):
        for key, name, n, q, mode, bits, fs, mi in shapes.matrix():
            gen_input(ref, name, n, q)
            gen_fit(ref, captured, key, name, n, q, mode, bits, fs, mi)
    ARR = {k: (np.stack(v) if k in ("xnew", "cdf") else np.concatenate(v)) for k, v in PACK.items()}
    save_npz(os.path.join(HERE, "ref_shapes.npz"), ARR)
    with open(os.path.join(HERE, "ref_shapes.json"), "w") as f:
        json.dump(MAN, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    fits = [c for c in MAN["cases"].values() if "n_iter" in c]
    cats = {}
    for k, c in sorted(MAN["cases"].items()):
        if "n_iter" in c:
            cat = shapes.category(c)
            cats.setdefault(cat, []).append(k)
    print(f"{len(MAN['cases'])} cases ({len(fits)} fits, {len(MAN['dropped'])} dropped), {len(ARR)} arrays,",
          os.path.getsize(os.path.join(HERE, "ref_shapes.npz")) // 1024, "KiB npz,",
          os.path.getsize(os.path.join(HERE, "ref_shapes.json")) // 1024, "KiB json")
    print({k: len(v) for k, v in cats.items()})
    for k in cats.get("divergent", []):
        c = MAN["cases"][k]
        if "/ternary/" not in k:
            print("divergent:", k, c["n_iter"], c["gap"], c["why"])
    print("dropped:", MAN["dropped"])


if __name__ == "__main__":
    main()
