"""An exact host restatement of scikit-learn 1.7.2's RandomForestClassifier(n_estimators, max_depth, random_state).fit on SNP codes
{0, 1, 2}: what gnx_train_rforest (forest/k_train_rforest.hip) must reproduce, tree for tree.  Plain numpy / Python.

The chain (sklearn/ensemble/_forest.py, sklearn/tree/_tree.pyx DepthFirstTreeBuilder, _splitter.pyx node_split_best, _criterion.pyx Gini):
  * forest: rs = RandomState(seed); tree seeds ts_t = rs.randint(2**31 - 1), n_trees draws in order;
  * tree t: bootstrap rows RandomState(ts_t).randint(0, N, N, dtype=int32) -> row weights bincount; the splitter's 32-bit state is a
    FRESH RandomState(ts_t).randint(0, 2147483647);
  * splitter generator our_rand_r: xorshift 13 / 17 / 5 on uint32 (state 0 becomes 1), returns state % 2^31;
    rand_int(lo, hi) = lo + r % (hi - lo);
  * depth-first builder, the left subtree first, node ids in pop order; a node is a leaf without a search if depth >= max_depth or
    its Gini impurity <= 2^-52 (a node of one distinct row is pure), and after a search if nothing split it (every drawn column
    constant) or improvement + 2^-52 < 0;
  * split search: the Fisher-Yates draw over the tree-global `features` permutation with `constant_features`, max_features =
    max(1, int(sqrt(width))); candidates between consecutive present codes, ascending; threshold lo / 2 + hi / 2; the proxy of the
    installed Criterion, -wR impR - wL impL, compared with a strict >;
  * every float64 expression is evaluated in scikit-learn's order, one IEEE operation per step (numpy float64 scalars, no fma).

A column is summarised per node by its weighted class counts for the codes 1 and 2 (code 0 follows from the node's class totals): the
device gets them from one int8 matrix product, scikit-learn from sorting the node's rows, and both then evaluate the same numbers.

fit_forest returns scikit-learn's tree arrays as they are (feature / threshold -2 at leaves); to_rf_arrays lays windows out as
convert.rforest_from_sklearn does (rf_feat 0 at leaves).  Each fit also counts the branches it took (COUNTER_NAMES)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)   # _tree.pyx EPSILON
RAND_R_MAX = 2147483647
COUNTER_NAMES = ("known_constant_drawn", "constant_found", "all_constant_search", "threshold_one", "leaf_above_max_depth")


def new_counters():
    return dict.fromkeys(COUNTER_NAMES, 0)


def tree_seeds(seed, n_trees):
    rs = np.random.RandomState(int(seed))
    return [int(rs.randint(np.iinfo(np.int32).max)) for _ in range(int(n_trees))]


def bootstrap(seed, n_trees, N):
    """-> (weights (n_trees, N) int64, splitter states (n_trees,) uint32) of RandomForestClassifier(random_state=seed) on N rows"""
    wt, st = np.zeros((int(n_trees), int(N)), np.int64), np.zeros(int(n_trees), np.uint32)
    for t, ts in enumerate(tree_seeds(seed, n_trees)):
        idx = np.random.RandomState(ts).randint(0, N, N, dtype=np.int32)
        wt[t] = np.bincount(idx, minlength=N)
        st[t] = np.random.RandomState(ts).randint(0, RAND_R_MAX)
    return wt, st


class _Rand:
    def __init__(self, state):
        self.s = int(state) & 0xFFFFFFFF

    def rand_int(self, lo, hi):
        s = self.s
        if s == 0:
            s = 1
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.s = s
        return lo + (s % (RAND_R_MAX + 1)) % (hi - lo)


def _gini(counts, w):
    sq = np.float64(0.0)
    for c in counts:
        c = np.float64(c)
        sq = sq + c * c
    return np.float64(1.0) - sq / (np.float64(w) * np.float64(w))


def fit_tree(X, y, A, weight, state, max_depth=4, counters=None):
    """one DecisionTreeClassifier(max_features="sqrt", max_depth).fit(X, y, sample_weight=weight) with the splitter state `state` ->
    dict children_left, children_right, feature, threshold (float64), value (n_nodes, A) — scikit-learn's tree_ arrays"""
    cnt = counters if counters is not None else new_counters()
    X = np.asarray(X)
    N, F = X.shape
    y = np.asarray(y)
    weight = np.asarray(weight, dtype=np.int64)
    rng = _Rand(state)
    max_features = max(1, int(np.sqrt(F)))
    features, constant = list(range(F)), [0] * F
    w_root = np.float64(weight.sum())
    left, right, feat, thr, value = [], [], [], [], []

    def counts_of(rows):
        return np.bincount(y[rows], weights=weight[rows], minlength=A).astype(np.int64)

    root_rows = np.flatnonzero(weight > 0)
    c0 = counts_of(root_rows)
    stack = [dict(rows=root_rows, depth=0, parent=-1, is_left=False, impurity=_gini(c0, c0.sum()), n_const=0, c=c0)]
    while stack:
        rec = stack.pop()
        rows, depth, c = rec["rows"], rec["depth"], rec["c"]
        w = np.float64(c.sum())
        is_leaf = depth >= max_depth or rec["impurity"] <= EPS
        best = None
        if not is_leaf:
            f_i, n_visited, n_found, n_drawn, n_known = F, 0, 0, 0, rec["n_const"]
            n_total = n_known
            best_proxy = -np.inf
            while f_i > n_total and (n_visited < max_features or n_visited <= n_found + n_drawn):
                n_visited += 1
                f_j = rng.rand_int(n_drawn, f_i - n_found)
                if f_j < n_known:
                    features[n_drawn], features[f_j] = features[f_j], features[n_drawn]
                    n_drawn += 1
                    cnt["known_constant_drawn"] += 1
                    continue
                f_j += n_found
                f = features[f_j]
                xs = X[rows, f]
                cv = [np.bincount(y[rows[xs == v]], weights=weight[rows[xs == v]], minlength=A).astype(np.int64) for v in (0, 1, 2)]
                present = [v for v in (0, 1, 2) if cv[v].sum() > 0]
                if len(present) < 2:
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    cnt["constant_found"] += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                L = np.zeros(A, np.int64)
                for lo, hi in zip(present[:-1], present[1:]):
                    L = L + cv[lo]
                    R = c - L
                    wL, wR = np.float64(L.sum()), np.float64(R.sum())
                    proxy = (-wR) * _gini(R, wR) - wL * _gini(L, wL)
                    if proxy > best_proxy:
                        best_proxy = proxy
                        t = np.float64(np.float32(lo)) / 2.0 + np.float64(np.float32(hi)) / 2.0
                        best = (f, t, L.copy(), R.copy())
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            rec["n_const"] = n_total
            if best is None:
                cnt["all_constant_search"] += 1
                is_leaf = True
            else:
                f, t, L, R = best
                wL, wR = np.float64(L.sum()), np.float64(R.sum())
                impL, impR = _gini(L, wL), _gini(R, wR)
                improvement = (w / w_root) * (rec["impurity"] - (wR / w * impR) - (wL / w * impL))
                is_leaf = improvement + EPS < 0.0
        node = len(left)
        if rec["parent"] >= 0:
            (left if rec["is_left"] else right)[rec["parent"]] = node
        value.append(c.astype(np.float64) / w)
        if is_leaf:
            left.append(-1); right.append(-1); feat.append(-2); thr.append(-2.0)
            if depth < max_depth:
                cnt["leaf_above_max_depth"] += 1
            continue
        left.append(-1); right.append(-1); feat.append(int(f)); thr.append(float(t))
        if t == 1.0:
            cnt["threshold_one"] += 1
        go_left = X[rows, f] <= t
        stack.append(dict(rows=rows[~go_left], depth=depth + 1, parent=node, is_left=False, impurity=impR, n_const=rec["n_const"], c=R))
        stack.append(dict(rows=rows[go_left], depth=depth + 1, parent=node, is_left=True, impurity=impL, n_const=rec["n_const"], c=L))
    return dict(children_left=np.array(left, np.int64), children_right=np.array(right, np.int64), feature=np.array(feat, np.int64),
                threshold=np.array(thr, np.float64), value=np.array(value, np.float64).reshape(-1, A))


def fit_forest(X, y, A, seed, n_trees=20, max_depth=4, counters=None):
    """RandomForestClassifier(n_estimators=n_trees, max_depth=max_depth, random_state=seed).fit(X, y) -> list of fit_tree dicts"""
    y = np.asarray(y)
    if sorted(set(y.tolist())) != list(range(A)):
        raise ValueError("y must hold every class of range(A)")
    wt, st = bootstrap(seed, n_trees, X.shape[0])
    return [fit_tree(X, y, A, wt[t], st[t], max_depth, counters) for t in range(int(n_trees))]


def window_columns(C, M, context, w):
    """columns of X that window w reads (reference base.py:41-44, 146-164: reflect padding, the last window wider by rem)"""
    W, rem = C // M, C - M * (C // M)
    width = M + 2 * context + (rem if w == W - 1 else 0)
    p = w * M + np.arange(width)
    return np.where(p < context, context - 1 - p, np.where(p < context + C, p - context, C - 1 - (p - context - C)))


def to_rf_arrays(forests):
    """per-window lists of tree dicts -> the rf_* arrays in convert.rforest_from_sklearn's layout"""
    wt0, off, L, R, F, T, V = [0], [0], [], [], [], [], []
    for trees in forests:
        for t in trees:
            L.append(t["children_left"].astype(np.int32)); R.append(t["children_right"].astype(np.int32))
            F.append(np.where(t["children_left"] == -1, 0, t["feature"]).astype(np.int32))
            T.append(t["threshold"].astype(np.float64)); V.append(t["value"].astype(np.float64))
            off.append(off[-1] + len(t["feature"]))
        wt0.append(len(off) - 1)
    return dict(rf_win_tree0=np.array(wt0, np.int32), rf_tree_off=np.array(off, np.int32), rf_left=np.concatenate(L),
                rf_right=np.concatenate(R), rf_feat=np.concatenate(F), rf_thr=np.concatenate(T), rf_value=np.concatenate(V))


def fit_windows(X, y, M, context, A, seeds, n_trees=20, max_depth=4, counters=None):
    """every window's forest on its padded slice, seeds (W,) -> rf_* arrays"""
    X, y = np.asarray(X), np.asarray(y)
    C = X.shape[1]
    W = C // M
    return to_rf_arrays([fit_forest(X[:, window_columns(C, M, context, w)], y[:, w], A, int(seeds[w]), n_trees, max_depth, counters)
                         for w in range(W)])


def identical_pairs(n_pairs, width, seed=0):
    """n_pairs pairs of identical rows with different labels: every node is impure, every column constant once a pair is alone"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 3, size=(n_pairs, width)).astype(np.int8)
    return np.repeat(base, 2, axis=0), np.tile(np.array([0, 1], np.int32), n_pairs)


def make_problem(A, width, N, seed):
    """codes {0, 1, 2} (2 rarer), an eighth of the columns duplicates of others, an eighth constant, labels correlated with a few
    columns, every class present"""
    rng = np.random.RandomState(seed)
    X = rng.choice(3, size=(N, width), p=[0.5, 0.35, 0.15]).astype(np.int8)
    y = (X[:, :5].sum(axis=1) + rng.randint(0, 2, N)) % A
    y[:A] = np.arange(A)
    k = max(1, width // 8)
    cols = rng.permutation(width)
    X[:, cols[:k]] = X[:, cols[k:2 * k]]
    X[:, cols[2 * k:3 * k]] = rng.randint(0, 3, k).astype(np.int8)
    # a few columns that hold 0s and 2s only (threshold 1.0)
    X[:, cols[3 * k:3 * k + 3]] = 2 * (X[:, cols[3 * k:3 * k + 3]] > 0)
    return X, y.astype(np.int32)


def window_labels(X, M, A, seed):
    """y (N, W): labels that follow a few SNPs of each window plus noise, every class present in every window"""
    rng = np.random.RandomState(seed)
    N, W = X.shape[0], X.shape[1] // M
    y = np.empty((N, W), np.int32)
    for w in range(W):
        y[:, w] = (X[:, w * M:w * M + 4].sum(axis=1) + rng.randint(0, 2, N)) % A
        y[:A, w] = np.arange(A)
    return y
