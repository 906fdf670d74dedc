"""gnx_simulate_admix(_dev) on the MI355X: bit-identical to the numpy expansion and to the reference's files (tests/golden/G21_sim),
the edge cases of the segment tables, the rejections, and the 7/8-argument command line end to end in fresh child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "G21_sim")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def plan():
    from gnomix_amd import simulate as S
    with open(os.path.join(G, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    return S.plan_splits(os.path.join(G, "panel.vcf.gz"), os.path.join(G, "gmap.tsv"), os.path.join(G, "smap.tsv"), cfg, chm="22")


def _call(ctx, F, off, beg, src, aof, A, N, C, M, ldx=None, want_anc=True):
    """host entry on explicit tables -> (rc, X, Y, anc)"""
    ldx = ldx or C
    X = np.full((max(N, 1), ldx), 77, np.int8)
    Y = np.full((max(N, 1), max(C // M, 1)), -7, np.int32)
    anc = np.full((max(N, 1), C), 99, np.uint8) if want_anc else None
    rc = ctx.lib.gnx_simulate_admix(ctx.h, F.ctypes.data, F.shape[0], F.shape[1], C, M, off.ctypes.data, beg.ctypes.data, src.ctypes.data,
                                    aof.ctypes.data, A, N, X.ctypes.data, ldx, Y.ctypes.data, anc.ctypes.data if want_anc else None)
    return rc, X, Y, anc


def _tables(segs):
    off, beg, src = [0], [], []
    for hap in segs:
        for b, s in hap:
            beg.append(b); src.append(s)
        off.append(len(beg))
    return np.array(off, np.int64), np.array(beg, np.int32), np.array(src, np.int32)


def test_kernel_equals_numpy_and_the_reference(ctx, plan):
    from gnomix_amd import simulate as S
    g = np.load(os.path.join(G, "expected.npz"))
    M = int(g["M"])
    X, Y, anc = plan.simulate_host(ctx, M)
    Xn, Yn, ancn = S.simulate_numpy(plan, M)
    assert np.array_equal(X, Xn) and np.array_equal(Y, Yn) and np.array_equal(anc, ancn)
    for split, gen, h0, n in plan.parts:
        key = "%s_gen%d" % (split, gen)
        assert np.array_equal(np.unpackbits(g["X_" + key], axis=1)[:, :plan.C], X[h0:h0 + n]), key
        assert np.array_equal(g["y_" + key], Y[h0:h0 + n]), key
    # the device form: founders built in HBM from the panel's 2-bit rows, every array a tensor
    Xd, Yd, ancd = plan.simulate_device(ctx, M)
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(Xd[:, :plan.C].cpu().numpy(), X) and np.array_equal(Yd.cpu().numpy(), Y) and np.array_equal(ancd.cpu().numpy(), anc)
    data = plan.materialise(ctx, M=M)
    assert np.array_equal(np.concatenate([d[0] for d in data]), X) and np.array_equal(np.concatenate([d[1] for d in data]), Y)


@pytest.mark.parametrize("C,ldx", [(100, 100), (333, 333), (333, 352), (4099, 4101), (8192, 8192)])
def test_edge_geometries(ctx, C, ldx):
    from gnomix_amd import simulate as S
    r = np.random.RandomState(C)
    nF, A, M = 10, 3, 7
    F = r.randint(0, 2, size=(nF, C)).astype(np.int8)
    aof = np.array([0, 0, 1, 1, 2, 2, S.NOT_A_FOUNDER, S.NOT_A_FOUNDER, 1, 0], np.uint8)
    segs = [[(0, 3)],                                             # no crossover
            [(0, 0), (16, 2), (32, 5)],                           # boundaries on 16-byte chunks
            [(0, 1), (5, 4), (17, 0), (C - 1, 9)],                # off chunks, a one-SNP last segment
            [(0, 5)] + [(b, int(r.choice([0, 1, 2, 3, 4, 5, 8, 9]))) for b in sorted(r.choice(np.arange(1, C), 12, replace=False))]]
    off, beg, src = _tables(segs)
    rc, X, Y, anc = _call(ctx, F, off, beg, src, aof, A, len(segs), C, M, ldx=ldx)
    assert rc == 0, ctx.lib.gnx_last_error(ctx.h)
    Xn, ancn = S.expand_numpy(F, off, beg, src, aof, C)
    assert np.array_equal(X[:, :C], Xn) and np.array_equal(anc, ancn)
    assert np.all(X[:, C:] == 77)                                 # padding of the rows untouched
    assert np.array_equal(Y, S.window_labels(ancn, M))
    rc, X2, Y2, _ = _call(ctx, F, off, beg, src, aof, A, len(segs), C, M, ldx=ldx, want_anc=False)
    assert rc == 0 and np.array_equal(X2, X) and np.array_equal(Y2, Y)


def test_rejections_are_error_codes(ctx):
    from gnomix_amd import _lib
    C, M, A = 64, 8, 2
    F = np.zeros((4, C), np.int8)
    aof = np.array([0, 0, 1, 1], np.uint8)
    ok = _tables([[(0, 0), (10, 2)], [(0, 1)]])
    assert _call(ctx, F, *ok, aof, A, 2, C, M)[0] == 0
    assert _call(ctx, F, *ok, aof, A, 0, C, M)[0] == 0                                      # N = 0: a no-op
    bad = [_tables([[(1, 0)], [(0, 1)]]),                                                   # first begin != 0
           _tables([[(0, 0), (10, 2), (10, 1)], [(0, 1)]]),                                 # begins not increasing
           _tables([[(0, 0), (C, 2)], [(0, 1)]]),                                           # begin >= C
           _tables([[(0, 0)], [(0, 4)]]),                                                   # source out of range
           _tables([[(0, 0)], [(0, -1)]]),
           (np.array([0, 1, 1], np.int64), np.array([0], np.int32), np.array([0], np.int32))]   # a haplotype without segments
    for off, beg, src in bad:
        rc = _call(ctx, F, off, beg, src, aof, A, 2, C, M)[0]
        assert rc == _lib.GNX_EINVAL, (off, beg, src)
    aof2 = np.array([0, 0, 255, 255], np.uint8)                                             # a row that is not a founder
    assert _call(ctx, F, *ok, aof2, A, 2, C, M)[0] == _lib.GNX_EINVAL
    assert _call(ctx, F, *ok, aof, 256, 2, C, M)[0] == _lib.GNX_EINVAL                       # A above GNX_SIM_MAX_A
    F2 = F.copy()
    F2[3, 40] = 2
    rc = _call(ctx, F2, *ok, aof, A, 2, C, M)[0]
    assert rc == _lib.GNX_EINVAL and "founder haplotype 3" in ctx.lib.gnx_last_error(ctx.h).decode()
    F2[3, 40] = 0
    F2[3, 41] = 0
    assert _call(ctx, F2, *ok, aof, A, 2, C, M)[0] == 0
    # the device form: the same verdicts, nothing written
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    X = torch.full((2, C), 5, dtype=torch.int8, device=dev)
    Y = torch.zeros((2, C // M), dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    off, beg, src = bad[1]
    rc = ctx.lib.gnx_simulate_admix_dev(ctx.h, t(F).data_ptr(), 4, C, C, M, t(off).data_ptr(), t(beg).data_ptr(), t(src).data_ptr(),
                                        t(aof).data_ptr(), A, 2, X.data_ptr(), C, Y.data_ptr(), None)
    assert rc == _lib.GNX_EINVAL and bool((X == 5).all())
    assert ctx.lib.gnx_simulate_admix_dev(ctx.h, None, 4, C, C, M, None, None, None, None, A, 0, None, C, None, None) == 0


def test_non_binary_founder_in_the_panel_names_sample_and_variant(ctx, plan, tmp_path):
    import gzip
    from gnomix_amd import _lib
    from gnomix_amd import simulate as S
    with gzip.open(os.path.join(G, "panel.vcf.gz"), "rt") as f:
        lines = f.read().splitlines()
    head = lines[2].split("\t")
    row = lines[10].split("\t")
    col = head.index("S007")
    row[col] = ".|1"
    lines[10] = "\t".join(row)
    p = tmp_path / "p.vcf"
    p.write_text("\n".join(lines) + "\n")
    with open(os.path.join(G, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    bad = S.plan_splits(str(p), os.path.join(G, "gmap.tsv"), os.path.join(G, "smap.tsv"), cfg, chm="22")
    with pytest.raises(_lib.GnxError) as e:
        bad.simulate_host(ctx, 9)
    assert "S007" in str(e.value) and "position %s" % row[1] in str(e.value)


def _run(args, cwd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py")] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_trains_saves_reloads_and_infers(tmp_path):
    cfg = os.path.join(G, "config.yaml")
    q = os.path.join(G, "panel.vcf.gz")
    out = tmp_path / "out"
    log = _run([q, str(out), "22", "False", os.path.join(G, "gmap.tsv"), q, os.path.join(G, "smap.tsv"), cfg], str(tmp_path))
    repo = out / "models" / "model_chm_22"
    for f in ("model_chm_22.gnx", "config.txt", "analysis/confusion_matrix_train.txt", "analysis/confusion_matrix_val.txt"):
        assert (repo / f).exists(), f
    for f in ("query_results.msp", "query_results.fb", "generated_data/metadata.pkl", "generated_data/train1/gen_24/mat_vcf_2d.npy"):
        assert (out / f).exists(), f
    acc = float(log.split("Estimated val accuracy: ")[1].split("%")[0])
    print("val smoother accuracy: %.2f %%" % acc)
    assert acc > 90.0, log                       # measured on an MI355X: 98.70 %
    assert "C\t500" in (repo / "config.txt").read_text()
    out2 = tmp_path / "reload"
    _run([q, str(out2), "22", "False", str(repo / "model_chm_22.gnx")], str(tmp_path))
    assert (out2 / "query_results.msp").read_bytes() == (out / "query_results.msp").read_bytes()
    # the same data read back from generated_data/ (simulation.run: False) trains the same model
    c2 = tmp_path / "c2.yaml"
    y = yaml.safe_load(open(cfg))
    y["simulation"]["run"], y["simulation"]["path"] = False, str(out / "generated_data")
    c2.write_text(yaml.safe_dump(y))
    out3 = tmp_path / "out3"
    _run(["None", str(out3), "22", "False", os.path.join(G, "gmap.tsv"), q, os.path.join(G, "smap.tsv"), str(c2)], str(tmp_path))
    assert (out3 / "models" / "model_chm_22" / "analysis" / "confusion_matrix_val.txt").read_bytes() == \
        (repo / "analysis" / "confusion_matrix_val.txt").read_bytes()


@pytest.mark.parametrize("mode,extra", [("fast", {}), ("large", {"max_ep": 5}), ("best", None)])
def test_cli_other_modes(tmp_path, mode, extra):
    y = yaml.safe_load(open(os.path.join(G, "config.yaml")))
    y["model"]["inference"] = mode
    y["simulation"]["rm_data"] = True
    if extra:
        y["model"]["smoother_kwargs"] = extra
    c = tmp_path / "c.yaml"
    c.write_text(yaml.safe_dump(y))
    q = os.path.join(G, "panel.vcf.gz")
    args = ["None", str(tmp_path / "out"), "22", "False", os.path.join(G, "gmap.tsv"), q, os.path.join(G, "smap.tsv"), str(c)]
    if mode == "best":
        r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py")] + args, cwd=str(tmp_path), capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 2 and '"best"' in r.stdout
        return
    _run(args, str(tmp_path))
    assert (tmp_path / "out" / "models" / "model_chm_22" / "model_chm_22.gnx").exists()
    assert not (tmp_path / "out" / "generated_data").exists()
