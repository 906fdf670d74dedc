#!/usr/bin/env python3
"""Generate tests/golden/G28_mode_filter.npz by RUNNING THE REFERENCE's mode_filter (src/Smooth/utils.py:31-46) through
np.apply_along_axis, as Smoother.predict does (src/Smooth/smooth.py:63-64), and — where pandas imports — its msp_to_lai and
msp_to_bed (src/postprocess.py:128-210) on one small .msp.  Run where the reference is present; it skips cleanly elsewhere.

The reference's mode() indexes stats.mode(arr)[0][0], which needs the array results scipy returned before 1.11.  On a newer scipy the
generator wraps scipy.stats.mode so that it is called with keepdims=True (scipy's own switch for the old shape): the wrapper wraps
scipy, the reference's text runs unchanged.

Stored: n_cases and, per case k, c<k>_in (N, W) int32, c<k>_size, c<k>_A, c<k>_out (N, W) int32 = the reference's labels.  For the
writers: w_labels (2 samples' worth of rows x W), w_chm / w_spos / w_epos / w_sgpos / w_egpos / w_nsnps, w_positions, w_samples,
w_pops, w_msp (the .msp text the reference read), w_lai (the .lai it wrote) and w_bed_names / w_bed_<i> (its .bed files).

The generator ASSERTS that the cases hold a two-way tie resolved to the centre, a tie whose centre is neither the smallest nor the
largest mode, a three-way tie, an unambiguous mode different from the centre, an even size, size 1, a size >= W and A = 2, and that
tests/labels_exact.py equals the reference on every case — otherwise the fixture would show nothing.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: labels_exact
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import make_golden as G  # noqa: E402  (import_reference)
import labels_exact as LE  # noqa: E402

OUT = os.path.join(HERE, "G28_mode_filter.npz")


def old_scipy_mode():
    """scipy.stats.mode returning arrays for a 1-d input, as scipy < 1.11 did"""
    import scipy
    from scipy import stats
    if tuple(int(x) for x in scipy.__version__.split(".")[:2]) < (1, 11):
        return
    plain = stats.mode

    def mode(a, *args, **kw):
        kw.setdefault("keepdims", True)
        return plain(a, *args, **kw)
    stats.mode = mode


def cases(rng):
    out = []
    hand = np.array([[0, 0, 1, 1, 2, 3, 3],      # size 5 at i = 2: {0, 1} tie, the centre 1 is the larger mode
                     [0, 0, 2, 1, 1, 3, 0],      # size 5 at i = 2: {0, 1} tie, the centre 2 is neither
                     [2, 1, 0, 3, 3, 0, 0],      # size 3 at i = 1: three-way tie
                     [1, 1, 0, 1, 2, 2, 2],      # size 3 at i = 2: mode 1, centre 0
                     [3, 3, 3, 3, 3, 3, 3]], np.int32)
    for size in (3, 5, 4, 1, 7, 8, 0, 2, 6):
        out.append((hand, size, 4))
    r5 = rng.randint(0, 5, size=(6, 40)).astype(np.int32)
    for size in (3, 5, 4, 9, 39, 40, 41, 100):
        out.append((r5, size, 5))
    smooth = np.repeat(rng.randint(0, 3, size=(4, 11)), 5, axis=1).astype(np.int32)[:, :53]   # runs with single-window flips
    flips = rng.rand(*smooth.shape) < 0.15
    smooth[flips] = rng.randint(0, 3, size=int(flips.sum()))
    for size in (3, 5, 11):
        out.append((smooth, size, 3))
    r2 = rng.randint(0, 2, size=(4, 33)).astype(np.int32)
    for size in (3, 5, 6):
        out.append((r2, size, 2))
    r32 = rng.randint(0, 32, size=(3, 50)).astype(np.int32)
    r32[1, 10:20] = 31
    for size in (3, 7):
        out.append((r32, size, 32))
    for W, size in ((1, 3), (4, 5), (5, 5), (6, 7), (7, 7), (2, 3), (3, 3)):   # W = 1, W = 2 ends, W = 2 ends + 1
        out.append((rng.randint(0, 3, size=(3, W)).astype(np.int32), size, 3))
    return out


def writer_inputs(rng):
    W, pops, samples = 5, ["AFR", "EUR", "NAT"], ["HG001", "NA.2"]
    labels = np.array([[0, 0, 0, 0, 0],      # one single run
                       [0, 1, 2, 1, 0],      # changes at every window
                       [2, 2, 1, 1, 1],
                       [1, 0, 0, 2, 2]], np.int32)
    spos = np.array([1000, 2000, 3000, 4000, 5000])
    epos = np.array([1990, 2990, 3990, 4990, 6370])
    sgpos = np.array([0.0, 0.51234, 1.25, 2.00001, 3.5])
    egpos = np.array([0.5, 1.2, 1.98765, 3.4, 4.75])
    nsnps = np.array([3, 2, 0, 4, 6])
    positions = np.sort(rng.choice(np.arange(900, 6500), size=int(nsnps.sum()), replace=False))
    return dict(labels=labels, chm=np.array(["22"] * W), spos=spos, epos=epos, sgpos=sgpos, egpos=egpos, nsnps=nsnps,
                positions=positions, samples=np.array(samples), pops=np.array(pops))


def msp_text(w):
    head = "#Subpopulation order/codes: " + "\t".join("%s=%d" % (p, i) for i, p in enumerate(w["pops"])) + "\n"
    head += "#chm\tspos\tepos\tsgpos\tegpos\tn snps\t" + "\t".join("%s.%d" % (s, h) for s in w["samples"] for h in (0, 1)) + "\n"
    rows = []
    for i in range(len(w["spos"])):
        rows.append("\t".join([str(w["chm"][i]), str(w["spos"][i]), str(w["epos"][i]), str(np.float64(w["sgpos"][i])),
                               str(np.float64(w["egpos"][i])), str(w["nsnps"][i])] + [str(v) for v in w["labels"][:, i]]))
    return head + "\n".join(rows) + "\n"


def main():
    if not G.import_reference():
        print("reference not present: nothing generated")
        return 0
    old_scipy_mode()
    from src.Smooth.utils import mode_filter
    rng = np.random.RandomState(2028)
    out, seen, sizes = {}, set(), set()
    cs = cases(rng)
    for k, (lab, size, A) in enumerate(cs):
        ref = np.apply_along_axis(func1d=mode_filter, axis=1, arr=lab, size=size) if size != 0 else lab
        assert np.array_equal(LE.mode_filter(lab, size), ref), "the restatement differs from the reference in case %d" % k
        assert lab.min() >= 0 and lab.max() < A
        ends, W = size // 2, lab.shape[1]
        if ends and 2 * ends < W:
            for row in lab:
                for i in range(ends, W - ends):
                    seen.add(LE.classify(row[i - ends:i + ends + 1], row[i]))
        sizes.add("even" if size and size % 2 == 0 else "one" if size == 1 else "ge_W" if size >= W else "odd")
        if size and size % 2 == 0 and size >= W:
            sizes.add("ge_W")
        if A == 2:
            sizes.add("A2")
        out.update({"c%d_in" % k: lab, "c%d_size" % k: np.int64(size), "c%d_A" % k: np.int64(A), "c%d_out" % k: ref.astype(np.int32)})
    out["n_cases"] = np.int64(len(cs))
    for need in ("tie2", "tie2_centre_between", "tie3", "mode_moves"):
        assert need in seen or (need == "tie3" and "tie3_centre_between" in seen), "no %s window in the cases" % need
    for need in ("even", "one", "ge_W", "A2"):
        assert need in sizes, "no case with %s" % need
    w = writer_inputs(rng)
    text = msp_text(w)
    out.update({"w_" + k: v for k, v in w.items()})
    out["w_msp"] = np.frombuffer(text.encode(), np.uint8)
    try:
        import pandas  # noqa: F401
        from src.postprocess import msp_to_bed, msp_to_lai
    except ImportError as e:
        print("pandas (or a package the reference's postprocess imports) is missing (%s): msp_to_lai / msp_to_bed NOT run" % e)
    else:
        with tempfile.TemporaryDirectory() as td:
            msp = os.path.join(td, "q.msp")
            with open(msp, "w") as f:
                f.write(text)
            msp_to_lai(msp, w["positions"], os.path.join(td, "q.lai"))
            out["w_lai"] = np.frombuffer(open(os.path.join(td, "q.lai"), "rb").read(), np.uint8)
            bed = os.path.join(td, "bed")
            os.makedirs(bed)
            msp_to_bed(msp, bed, pop_order=list(w["pops"]))
            # (the reference keeps the header line's newline in the last column's name: the file name is stored without it)
            names = sorted(os.listdir(bed))
            out["w_bed_names"] = np.array([n.replace("\n", "") for n in names])
            for i, n in enumerate(names):
                out["w_bed_%d" % i] = np.frombuffer(open(os.path.join(bed, n), "rb").read(), np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d filter cases, decisions seen %s, %s" % (OUT, len(cs), sorted(seen), sorted(sizes)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
