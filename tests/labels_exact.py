"""The label stages after the smoother's argmax restated in plain Python: the mode filter and the run list of a haplotype.

What gnomix_amd/csrc/labels/k_labels.hip must reproduce EXACTLY (its header states the same rules):
  mode_filter(pred, size): ends = size // 2; position i with ends <= i < W - ends (none when ends == 0 or 2 * ends >= W) becomes the
    most frequent label of pred[i - ends .. i + ends] when the smallest and the largest most frequent label are the same label, and
    stays pred[i] otherwise; the windows are read from the input row; size 0 / None / False changes nothing.
  label_runs(labels): per row the maximal stretches of equal labels as (first_window, last_window, label), row after row, with the
    rows' run counts and their exclusive prefix.
Nothing here imports the package under test."""
import numpy as np


def window_verdict(window, centre):
    """the filter's value for one window: its mode when unambiguous, else the centre"""
    counts = {}
    for v in window:
        counts[int(v)] = counts.get(int(v), 0) + 1
    best = max(counts.values())
    modes = [v for v, c in counts.items() if c == best]
    lo, hi = min(modes), max(modes)
    return lo if lo == hi else int(centre)


def mode_filter_row(pred, size):
    pred = [int(v) for v in pred]
    out = list(pred)
    if not size:
        return out
    ends = int(size) // 2
    W = len(pred)
    if ends == 0 or 2 * ends >= W:
        return out
    for i in range(ends, W - ends):
        out[i] = window_verdict(pred[i - ends:i + ends + 1], pred[i])
    return out


def mode_filter(labels, size):
    """labels (N, W) ints -> filtered copy, same dtype"""
    labels = np.asarray(labels)
    out = labels.copy()
    for n in range(labels.shape[0]):
        out[n] = mode_filter_row(labels[n], size)
    return out


def classify(window, centre):
    """what kind of decision a window is, for the fixture generator's assertions:
    'mode' (one mode, equal to the centre), 'mode_moves' (one mode, not the centre), 'tie2' / 'tie3' (that many modes; the centre
    stays), with '_centre_between' appended when the centre is neither the smallest nor the largest mode"""
    counts = {}
    for v in window:
        counts[int(v)] = counts.get(int(v), 0) + 1
    best = max(counts.values())
    modes = sorted(v for v, c in counts.items() if c == best)
    if len(modes) == 1:
        return "mode" if modes[0] == int(centre) else "mode_moves"
    kind = "tie2" if len(modes) == 2 else "tie3" if len(modes) == 3 else "tie_many"
    return kind + ("_centre_between" if int(centre) not in (modes[0], modes[-1]) else "")


def label_runs(labels):
    """labels (N, W) ints -> (counts (N,) int64, offsets (N + 1,) int64, triples (total, 3) int32)"""
    labels = np.asarray(labels)
    N, W = labels.shape
    counts, triples = np.zeros(N, np.int64), []
    for n in range(N):
        start = 0
        for w in range(1, W + 1):
            if w == W or labels[n, w] != labels[n, start]:
                if W > 0:
                    triples.append((start, w - 1, int(labels[n, start])))
                    counts[n] += 1
                start = w
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return counts, offsets, np.asarray(triples, dtype=np.int32).reshape(-1, 3)
