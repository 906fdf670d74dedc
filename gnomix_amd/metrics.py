"""The two scores the reference's evaluate() methods print (src/Base/base.py:214-228, src/Smooth/smooth.py:67-79: sklearn's
accuracy_score and balanced_accuracy_score, in percent, rounded to two decimals) and its confusion matrix
(src/model.py:93-98), in numpy."""
from __future__ import annotations

import numpy as np


def confusion(y, y_pred):
    """(matrix over the sorted union of labels, those labels) — sklearn.metrics.confusion_matrix's default label set"""
    y = np.asarray(y).reshape(-1)
    y_pred = np.asarray(y_pred).reshape(-1)
    labels = np.unique(np.concatenate([y, y_pred]))
    idx = {int(l): i for i, l in enumerate(labels)}
    cm = np.zeros((len(labels), len(labels)), dtype=np.int64)
    np.add.at(cm, (np.searchsorted(labels, y), np.searchsorted(labels, y_pred)), 1)
    return cm, [int(l) for l in labels]


def _pair(acc, cm):
    support = cm.sum(axis=1)
    recall = np.diag(cm)[support > 0] / support[support > 0]
    return round(acc * 100, 2), round(float(np.mean(recall)) * 100, 2)


def accuracy_pair(y, y_pred):
    """(accuracy, balanced accuracy) in percent, two decimals.  Balanced = mean recall over the classes present in y."""
    y = np.asarray(y).reshape(-1)
    y_pred = np.asarray(y_pred).reshape(-1)
    acc = float(np.mean(y == y_pred))
    cm, labels = confusion(y, y_pred)
    return _pair(acc, cm)


# ---- the same three from the A x A counts  counts[t, p] = #{y == t and y_pred == p}  over the labels 0 .. A-1 (what gnx_confusion_dev
# returns for a split predicted on the device): equal to the label-vector forms above, value for value
def confusion_from_counts(counts):
    """confusion(y, y_pred): the rows and columns of the labels that occur in y or in y_pred (a label neither true nor predicted
    anywhere is not in the sorted union, so it has no row), and those labels"""
    counts = np.asarray(counts, dtype=np.int64)
    labels = np.flatnonzero((counts.sum(axis=1) + counts.sum(axis=0)) > 0)
    return np.ascontiguousarray(counts[np.ix_(labels, labels)]), [int(l) for l in labels]


def accuracy_pair_from_counts(counts):
    """accuracy_pair(y, y_pred): the mean of (y == y_pred) is trace / n, both exact integers in float64, so the quotient is the same
    float; the recalls are those of the classes with a true label (a class absent from y has support 0 and is left out, as
    balanced_accuracy_score leaves it out; a class never predicted has recall 0 and counts)"""
    counts = np.asarray(counts, dtype=np.int64)
    acc = float(np.float64(np.trace(counts)) / counts.sum())
    cm, _ = confusion_from_counts(counts)
    return _pair(acc, cm)
