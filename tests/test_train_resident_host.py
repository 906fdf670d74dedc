"""The host half of training from device-resident splits (no GPU): the reference's accuracy, balanced accuracy and confusion
matrix computed from A x A counts equal the label-vector forms of gnomix_amd/metrics.py; CUDA tensors and numpy arrays do not
mix; the library exports the confusion entries and the new kernel carries no scratch."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(y, p, A):
    c = np.zeros((A, A), np.int64)
    np.add.at(c, (y, p), 1)
    return c


# A, a class absent from y, a class never predicted
CASES = [(3, None, None), (4, 2, None), (4, None, 1), (5, 0, 4), (5, 3, 3), (2, None, None), (2, 1, None), (7, 6, 0)]


@pytest.mark.parametrize("A,absent,never", CASES)
def test_scores_from_counts_equal_scores_from_label_vectors(A, absent, never):
    from gnomix_amd import metrics
    rng = np.random.RandomState(17 * A + (absent or 0) + 3 * (never or 0))
    for n in (1, 37, 4001):
        y, p = rng.randint(0, A, n), rng.randint(0, A, n)
        p = np.where(rng.random_sample(n) < 0.6, y, p)             # mostly right, as a trained model is
        if absent is not None:
            y = np.where(y == absent, (absent + 1) % A, y)
        if never is not None:
            p = np.where(p == never, (never + 2) % A, p)
        counts = _counts(y, p, A)
        assert metrics.accuracy_pair_from_counts(counts) == metrics.accuracy_pair(y, p)
        cm, labels = metrics.confusion(y, p)
        cm_c, labels_c = metrics.confusion_from_counts(counts)
        assert labels_c == labels and cm_c.dtype == cm.dtype and np.array_equal(cm_c, cm)
        if absent is not None and (never == absent or not np.any(p == absent)):
            assert absent not in labels_c                          # neither true nor predicted: the reference's matrix has no row for it


def test_a_class_absent_from_y_is_left_out_of_the_balanced_accuracy():
    """balanced_accuracy_score averages the recall over the classes that occur in y_true: class 2 is predicted but never true"""
    from gnomix_amd import metrics
    y, p = np.array([0, 0, 0, 1, 1, 1]), np.array([0, 0, 2, 1, 2, 2])
    assert metrics.accuracy_pair(y, p) == (50.0, 50.0)             # recalls 2/3 and 1/3; a zero recall for class 2 would give 33.33
    assert metrics.accuracy_pair_from_counts(_counts(y, p, 3)) == (50.0, 50.0)
    assert metrics.confusion_from_counts(_counts(y, p, 4))[1] == [0, 1, 2]


def test_host_arrays_and_cuda_tensors_do_not_mix():
    from gnomix_amd import resident

    class FakeCuda:
        is_cuda = True

    a = np.zeros(3)
    assert resident.all_on_device([a, a, None]) is False and resident.all_on_device([None, None]) is False
    assert resident.all_on_device([FakeCuda(), None, FakeCuda()]) is True
    with pytest.raises(TypeError, match="mixes host arrays and CUDA tensors"):
        resident.all_on_device([a, FakeCuda()])
    import torch
    assert resident.is_cuda(torch.zeros(2)) is False                # a CPU tensor is host data


def test_command_line_trains_resident_only_in_default_mode_without_kept_data():
    from gnomix_amd.cli import train_resident
    from gnomix_amd.simulate import merge_config

    def cfg(mode="default", rm_data=True, run=True, path=None):
        c = merge_config({"simulation": {"rm_data": rm_data, "run": run, "path": path}, "model": {"inference": mode}})
        return c

    assert train_resident(cfg(), environ={}) is True
    assert train_resident(merge_config({}), environ={}) is False          # the default keeps generated_data: host arrays
    assert train_resident(cfg(rm_data=False), environ={}) is False
    assert train_resident(cfg(mode="fast"), environ={}) is False
    assert train_resident(cfg(mode="large"), environ={}) is False
    assert train_resident(cfg(run=False, path="/some/generated_data"), environ={}) is False
    assert train_resident(cfg(), environ={"GNX_TRAIN_RESIDENT": "0"}) is False
    assert train_resident(cfg(), environ={"GNX_TRAIN_RESIDENT": "1"}) is True
    assert train_resident(cfg(), environ={"GNX_NO_TORCH": "1"}) is False


def test_adjacent_rows_of_one_allocation_are_one_view():
    import torch
    from gnomix_amd import resident
    X = torch.arange(10 * 16, dtype=torch.int8).reshape(10, 16)
    parts = [X[0:4, :13], X[4:7, :13], X[7:10, :13]]
    V = resident.adjacent_rows(parts)
    assert V.data_ptr() == X.data_ptr() and tuple(V.shape) == (10, 13) and V.stride() == (16, 1) and torch.equal(V, X[:, :13])
    assert resident.adjacent_rows([parts[0], parts[2]]) is None
    assert resident.adjacent_rows([parts[1], parts[0]]) is None
    assert resident.adjacent_rows([parts[0], X[4:7, :12]]) is None
    assert resident.adjacent_rows([parts[0], parts[1].clone()]) is None


def test_library_exports_the_confusion_entries_without_scratch():
    from gnomix_amd import _lib
    lib = _lib.load()
    assert "gnx_confusion_dev" in _lib.SYMBOLS and "gnx_confusion" in _lib.SYMBOLS
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16     # an addition: the ABI version stays
    spec = importlib.util.spec_from_file_location("scratch_audit", os.path.join(ROOT, "scripts", "scratch_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    ks = [k for k in audit.kernels() if k["name"].startswith("k_confusion<")]
    assert len(ks) == 3                                            # labels, float64 rows, float32 rows
    for k in ks:
        assert k["scratch"] == 0 and k["lds"] == (32 * 32 + 1) * 4, k
        assert any(re.search(p, k["name"]) for p in audit.MUST_BE_CLEAN)
    assert audit.main(["--check"]) == 0
