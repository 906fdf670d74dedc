"""Converters: reference objects -> GnxModelData (the export a maintainer runs once per model.pkl).

`from_reference_model` needs the packages the pickle itself needs (sklearn, and xgboost or
sklearn_crfsuite for the smoother): they are only touched through public fitted attributes.
`trees_from_xgb_json` parses xgboost's documented JSON dump (Booster.get_dump(dump_format="json")),
so it is testable without xgboost installed."""
from __future__ import annotations

import json

import numpy as np

from .model import GnxModelData


def cov_sample(width, alpha=0.6, beta=1.0, seed=37):
    """Substring lengths of the covering random string kernel for a window of `width` SNPs
    (reference src/Base/string_kernel.py:80-89: legacy MT19937 stream seeded per call, one uniform draw
    per m = 2..width).  The sequence is prefix-stable in `width`."""
    rs = np.random.RandomState(seed)
    ms = [1]
    for m in range(2, int(width) + 1):
        if (1 - (alpha ** (m - ms[-1] + 1))) * (m ** (-beta)) >= rs.random_sample():
            ms.append(m)
    return np.asarray(ms, dtype=np.int32)


def string_kernel_lengths(width, kernel_name="CovRSK"):
    """Substring lengths the window kernel counts: the covering sample for CovRSKBase, every length 1..width for the
    plain triangular-number kernel of StringKernelBase (string_kernel.py:5-24: K = sum over runs L(L+1)/2)."""
    if "CovRSK" in kernel_name:
        return cov_sample(width)
    if "string_kernel" in kernel_name:
        return np.arange(1, int(width) + 1, dtype=np.int32)
    raise NotImplementedError(f"string kernel {kernel_name}")


def svc_window_from_sklearn(svc, width, kernel_name="CovRSK"):
    """One fitted sklearn.svm.SVC(probability=True) -> the dict GnxModelData.svc holds: kernel=callable (the string-kernel bases)
    or kernel="rbf" (SVMBase, src/Base/models.py:148-159)."""
    if isinstance(getattr(svc, "kernel", None), str):
        if svc.kernel != "rbf":
            raise NotImplementedError(f"SVC kernel {svc.kernel!r}: only 'rbf' (SVMBase) and the string kernels are built")
        return svc_rbf_window_from_sklearn(svc, width)
    xfit = getattr(svc, "_BaseLibSVM__Xfit")
    d = dict(xfit=np.ascontiguousarray(xfit, dtype=np.int8), support=svc.support_.astype(np.int32),
             dual_coef=np.ascontiguousarray(svc._dual_coef_, dtype=np.float64),
             intercept=np.ascontiguousarray(svc._intercept_, dtype=np.float64),
             prob_a=np.ascontiguousarray(svc._probA, dtype=np.float64),
             prob_b=np.ascontiguousarray(svc._probB, dtype=np.float64),
             n_support=svc._n_support.astype(np.int32))
    if "poly" in kernel_name:   # PolynomialStringKernelBase (models.py:178-193): poly_kernel(X, Y, p=1.2)
        d.update(poly_run_values(width))
    else:
        d["ms"] = string_kernel_lengths(width, kernel_name)
    return d


def svc_rbf_window_from_sklearn(svc, width):
    """One fitted SVC(kernel="rbf", probability=True) -> an RBF window dict.  Only the support rows are kept (support_vectors_,
    float64 in sklearn: they must be whole numbers in 0..2, the SNP codes), gamma is the fitted _gamma."""
    sv = np.asarray(svc.support_vectors_)
    if hasattr(sv, "toarray"):
        sv = sv.toarray()
    sv = np.asarray(sv, dtype=np.float64)
    if sv.ndim != 2 or sv.shape[1] != int(width):
        raise ValueError(f"support_vectors_ must be (n_sv, {int(width)}), got {sv.shape}")
    if not np.all(np.isfinite(sv)) or np.any(sv != np.rint(sv)) or sv.min() < 0 or sv.max() > 2:
        raise ValueError("support_vectors_ must hold the SNP codes 0, 1, 2 (whole numbers): the RBF base computes |x - y|^2 "
                         "in integers")
    gamma = float(svc._gamma)
    if not (np.isfinite(gamma) and gamma > 0):
        raise ValueError(f"_gamma must be finite and > 0, got {gamma}")
    n = sv.shape[0]
    return dict(xfit=np.ascontiguousarray(sv, dtype=np.int8), support=np.arange(n, dtype=np.int32),
                dual_coef=np.ascontiguousarray(svc._dual_coef_, dtype=np.float64),
                intercept=np.ascontiguousarray(svc._intercept_, dtype=np.float64),
                prob_a=np.ascontiguousarray(svc._probA, dtype=np.float64),
                prob_b=np.ascontiguousarray(svc._probB, dtype=np.float64),
                n_support=np.asarray(svc._n_support).astype(np.int32), kernel=np.array("rbf"), gamma=np.float64(gamma))


def knn_window_from_sklearn(knn, width, n_class):
    """One fitted KNeighborsClassifier(n_neighbors=1) (or a stubbed pickle's attribute bag with the same attributes) -> the dict
    GnxModelData.knn holds: xfit = _fit_X as int8, y = classes_[_y] as int32.  Refused: n_neighbors != 1, non-uniform weights,
    a metric other than Euclidean (Minkowski with p = 2), fit data that are not the whole-number SNP codes 0..2 (the kernel's
    distances are integers), labels outside 0..n_class-1."""
    k = getattr(knn, "n_neighbors", None)
    if k is None or int(k) != 1:
        raise NotImplementedError(f"KNeighborsClassifier with n_neighbors = {k!r}: only n_neighbors = 1 (KNNBase) is built")
    wts = getattr(knn, "weights", "uniform")
    if wts is not None and (not isinstance(wts, str) or wts != "uniform"):
        raise NotImplementedError(f"KNeighborsClassifier with weights = {wts!r}: only uniform weights are built")
    metric, p = getattr(knn, "metric", "minkowski"), getattr(knn, "p", 2)
    eff = getattr(knn, "effective_metric_", None)
    euclid = (isinstance(metric, str) and metric in ("euclidean", "l2")) or \
             (isinstance(metric, str) and metric == "minkowski" and p is not None and float(p) == 2.0)
    if not euclid or (eff is not None and eff not in ("euclidean", "l2", "minkowski")):
        raise NotImplementedError(f"KNeighborsClassifier with metric = {metric!r}, p = {p!r}: only the Euclidean metric "
                                  "(minkowski, p = 2) is built")
    fx = knn._fit_X
    if hasattr(fx, "toarray"):
        fx = fx.toarray()
    fx = np.asarray(fx)
    if fx.ndim != 2 or fx.shape[1] != int(width) or fx.shape[0] < 1:
        raise ValueError(f"_fit_X must be (n_fit >= 1, {int(width)}), got {fx.shape}")
    f64 = fx.astype(np.float64)
    if not np.all(np.isfinite(f64)) or np.any(f64 != np.rint(f64)) or f64.min() < 0 or f64.max() > 2:
        raise ValueError("_fit_X must hold the SNP codes 0, 1, 2 (whole numbers): the 1-NN base computes |x - y|^2 in integers")
    classes = np.asarray(knn.classes_)
    yi = np.asarray(knn._y).reshape(-1)
    if len(yi) != fx.shape[0] or yi.min() < 0 or yi.max() >= len(classes):
        raise ValueError("_y must index classes_ for every row of _fit_X")
    lab = classes[yi]
    if np.any(lab != np.rint(np.asarray(lab, dtype=np.float64))) or lab.min() < 0 or lab.max() >= int(n_class):
        raise ValueError(f"classes_ must be whole numbers in 0..{int(n_class) - 1}, got {classes.tolist()}")
    return dict(xfit=np.ascontiguousarray(f64, dtype=np.int8), y=np.ascontiguousarray(lab, dtype=np.int32))


NB_KINDS = {"BernoulliNB": "bernoulli", "MultinomialNB": "multinomial", "GaussianNB": "gaussian"}


def nb_tables(kind, attrs, n_class):
    """fitted attributes of ONE window -> (table (width, 4, A), bias (A,)) float64 as gnx_nb_window takes them.  attrs: classes_ and,
    for "bernoulli" / "multinomial", feature_log_prob_ (k, width) and class_log_prior_ (k,); for "gaussian" theta_, var_ (k, width)
    and class_prior_ (k,).  Class column c = classes_[k]; a class absent from classes_ gets bias -inf and zero table rows.
      bernoulli:    T[p,0,c] = log(1 - exp(flp[c,p])), T[p,v>=1,c] = flp[c,p];  bias = class_log_prior_
      multinomial:  T[p,v,c] = v * flp[c,p];                                    bias = class_log_prior_
      gaussian:     T[p,v,c] = -0.5 (v - theta_[c,p])^2 / var_[c,p];           bias = log(class_prior_) - 0.5 sum_p log(2 pi var_)
    (scikit-learn's _joint_log_likelihood of each estimator, evaluated at the four codes.)"""
    A = int(n_class)
    classes = np.asarray(attrs["classes_"])
    cf = np.asarray(classes, dtype=np.float64)
    if classes.ndim != 1 or len(classes) < 1 or np.any(cf != np.rint(cf)) or cf.min() < 0 or cf.max() >= A or len(set(cf.tolist())) != len(cf):
        raise ValueError(f"classes_ must be distinct whole numbers in 0..{A - 1}, got {classes.tolist()}")
    cols = cf.astype(np.int64)
    v = np.arange(4, dtype=np.float64)
    if kind in ("bernoulli", "multinomial"):
        flp = np.asarray(attrs["feature_log_prob_"], dtype=np.float64)
        prior = np.asarray(attrs["class_log_prior_"], dtype=np.float64).reshape(-1)
        if flp.ndim != 2 or flp.shape[0] != len(cols) or prior.shape != (len(cols),):
            raise ValueError("feature_log_prob_ must be (n_classes, width) and class_log_prior_ (n_classes,)")
        if not np.all(np.isfinite(flp)):
            raise ValueError("feature_log_prob_ is not finite: alpha=0 under scikit-learn >= 1.4 leaves log 0 on a class-monomorphic SNP "
                             "(no smoothing is applied), and scikit-learn itself then returns NaN probabilities; refit with alpha > 0 "
                             "(scikit-learn <= 1.3 raised alpha=0 to 1e-10, which gnomix_amd.train.train_nb_base does)")
        if kind == "bernoulli":
            with np.errstate(divide="ignore"):
                neg = np.log(1.0 - np.exp(flp))
            if not np.all(np.isfinite(neg)):
                raise ValueError("log(1 - exp(feature_log_prob_)) is not finite: a SNP is non-zero in every row of a class and no "
                                 "smoothing was applied (alpha=0 under scikit-learn >= 1.4 leaves log 0 there, and scikit-learn itself "
                                 "then returns NaN probabilities); refit with alpha > 0")
            t = np.stack([neg, flp, flp, flp], axis=0)                      # (4, k, width)
        else:
            t = v[:, None, None] * flp[None]
        b = prior
    elif kind == "gaussian":
        theta = np.asarray(attrs["theta_"], dtype=np.float64)
        var = np.asarray(attrs["var_"], dtype=np.float64)
        cp = np.asarray(attrs["class_prior_"], dtype=np.float64).reshape(-1)
        if theta.ndim != 2 or theta.shape != var.shape or theta.shape[0] != len(cols) or cp.shape != (len(cols),):
            raise ValueError("theta_ / var_ must be (n_classes, width) and class_prior_ (n_classes,)")
        if not (np.all(np.isfinite(theta)) and np.all(np.isfinite(var)) and np.all(var > 0) and np.all(np.isfinite(cp)) and np.all(cp > 0)):
            raise ValueError("theta_ / var_ / class_prior_ must be finite, var_ and class_prior_ positive")
        t = -0.5 * (v[:, None, None] - theta[None]) ** 2 / var[None]
        b = np.log(cp) - 0.5 * np.sum(np.log(2.0 * np.pi * var), axis=1)
    else:
        raise ValueError(f"nb kind must be one of {sorted(NB_KINDS.values())}, got {kind!r}")
    if not np.all(np.isfinite(t)) or not np.all(np.isfinite(b)):
        raise ValueError("the Naive-Bayes table / bias of a present class is not finite")
    width = t.shape[2]
    table = np.zeros((width, 4, A))
    bias = np.full(A, -np.inf)
    table[:, :, cols] = np.transpose(t, (2, 0, 1))
    bias[cols] = b
    return table, bias


def nb_window_from_sklearn(nb, width, n_class, kind=None):
    """One fitted BernoulliNB / MultinomialNB / GaussianNB (or a stubbed pickle's attribute bag with the same attributes; then pass
    `kind`) -> (table (width, 4, A), bias (A,)).  Refused: BernoulliNB with binarize != 0.0 (ValueError), non-finite
    feature_log_prob_ (ValueError: see nb_tables), a width that is not the window's."""
    kind = kind or NB_KINDS.get(type(nb).__name__)
    if kind is None:
        raise NotImplementedError(f"{type(nb).__name__} is not a Naive-Bayes estimator this library converts")
    if kind == "bernoulli":
        bz = getattr(nb, "binarize", 0.0)
        if bz is None or float(bz) != 0.0:
            raise ValueError(f"BernoulliNB with binarize = {bz!r}: only binarize = 0.0 (a SNP code counts as set when it is non-zero) is built")
    names = ("classes_", "feature_log_prob_", "class_log_prior_") if kind != "gaussian" else ("classes_", "theta_", "var_", "class_prior_")
    attrs = {}
    for k in names:
        if not hasattr(nb, k) and k == "var_" and hasattr(nb, "sigma_"):   # scikit-learn < 1.0 named it sigma_
            attrs[k] = nb.sigma_
        else:
            attrs[k] = getattr(nb, k)
    table, bias = nb_tables(kind, attrs, n_class)
    if table.shape[0] != int(width):
        raise ValueError(f"the estimator was fitted on {table.shape[0]} features, the window is {int(width)} wide")
    return table, bias


def lda_from_sklearn(m, width, n_class=None):
    """One fitted LinearDiscriminantAnalysis (or a stubbed pickle's attribute bag with the same attributes) -> (coef (A or 1, width),
    intercept (A or 1,)) float64 as gnx_lda_window takes them: coef_ and intercept_ as scikit-learn keeps them (for two classes the one
    row coef_[1] - coef_[0]).  Refused (ValueError): a solver other than "svd", shrinkage, classes_ that are not 0 .. A-1 (the
    reference's vectorized path has no remap), a width that is not the window's, non-finite values."""
    solver = getattr(m, "solver", "svd")
    if solver != "svd":
        raise ValueError(f"LinearDiscriminantAnalysis with solver = {solver!r}: only the default \"svd\" (what LDABase builds) is converted")
    if getattr(m, "shrinkage", None) is not None:
        raise ValueError(f"LinearDiscriminantAnalysis with shrinkage = {m.shrinkage!r}: LDABase builds none")
    classes = np.asarray(m.classes_)
    A = int(n_class) if n_class is not None else len(classes)
    if classes.ndim != 1 or len(classes) != A or np.any(np.asarray(classes, dtype=np.float64) != np.arange(A)):
        raise ValueError(f"classes_ != 0..{A - 1} (the vectorized reference path has no remap, base.py:176), got {classes.tolist()}")
    coef = np.asarray(m.coef_, dtype=np.float64)
    icpt = np.asarray(m.intercept_, dtype=np.float64).reshape(-1)
    R = 1 if A == 2 else A
    if coef.ndim != 2 or coef.shape[0] != R or icpt.shape != (R,):
        raise ValueError(f"coef_ must be ({R}, width) and intercept_ ({R},) for {A} classes, got {coef.shape} and {icpt.shape}")
    if coef.shape[1] != int(width):
        raise ValueError(f"the estimator was fitted on {coef.shape[1]} features, the window is {int(width)} wide")
    if not (np.all(np.isfinite(coef)) and np.all(np.isfinite(icpt))):
        raise ValueError("coef_ / intercept_ is not finite")
    return np.ascontiguousarray(coef), icpt


def poly_run_values(width, p=1.2):
    """what a run of L equal SNPs contributes to the polynomial string kernel (string_kernel.py:52: contigs ** p), computed
    by numpy exactly as the reference computes it (int64 array ** float)"""
    return dict(poly_p=float(p), run_value=np.arange(int(width) + 1, dtype=np.int64) ** p)


def trees_from_xgb_json(dumps, n_class, base_score=0.5):
    """xgboost JSON tree dumps (list of str, one per tree, model order) -> xgboost-schema arrays.
    JSON nodes: {"nodeid", "split": "f12", "split_condition", "yes", "no", "missing", "children"} or {"nodeid","leaf"};
    `yes` is the child taken when feature < split_condition."""
    off, L, R, F, Cd, Dl, cls = [0], [], [], [], [], [], []
    for t, s in enumerate(dumps):
        root = json.loads(s) if isinstance(s, str) else s
        nodes = {}

        def visit(nd):
            nodes[nd["nodeid"]] = nd
            for ch in nd.get("children", []):
                visit(ch)

        visit(root)
        ids = sorted(nodes)
        remap = {nid: k for k, nid in enumerate(ids)}
        if remap[root["nodeid"]] != 0:
            raise ValueError("tree root must have the smallest node id")
        for nid in ids:
            nd = nodes[nid]
            if "leaf" in nd:
                L.append(-1); R.append(-1); F.append(0); Cd.append(np.float32(nd["leaf"])); Dl.append(0)
            else:
                f = nd["split"]
                f = int(f[1:]) if isinstance(f, str) and f.startswith("f") else int(f)
                L.append(remap[nd["yes"]]); R.append(remap[nd["no"]]); F.append(f)
                Cd.append(np.float32(nd["split_condition"]))
                Dl.append(int(nd.get("missing", nd["yes"]) == nd["yes"]))
        off.append(len(L))
        cls.append(t % n_class)
    return dict(tree_off=np.array(off, np.int32), left=np.array(L, np.int32), right=np.array(R, np.int32),
                feat=np.array(F, np.int32), cond=np.array(Cd, np.float32), tree_class=np.array(cls, np.int32),
                base_score=float(base_score), default_left=np.array(Dl, np.uint8))


def xgb_trees_of(xgb_obj, n_class):
    """xgboost-schema arrays of a fitted XGBClassifier.  Always through the booster's own serialised model
    (gnomix_amd.refpickle.parse_xgb_raw): the raw bytes a stubbed pickle carries, or `Booster.save_raw()` of a real
    object — so trees-per-round, tree_info (the class of every tree) and base_score come from the booster itself and are
    never guessed from A (an A == 2 smoother trained as multi:softprob num_class=2, src/Smooth/models.py:14-20, has two
    trees per round; XGBBase with A == 2 is binary:logistic with one)."""
    from .refpickle import booster_bytes, parse_xgb_raw
    raw = booster_bytes(xgb_obj)
    if raw is None:
        booster = xgb_obj.get_booster()
        try:
            raw = booster.save_raw(raw_format="json")   # xgboost >= 1.6
        except TypeError:
            raw = booster.save_raw()                     # xgboost 1.1.1: legacy binary
    t = parse_xgb_raw(bytes(raw))
    n_out = max(int(t["n_class"]), 1)
    if n_out > 1 and n_out != n_class:
        raise ValueError(f"xgboost model: num_class={n_out} but the Gnomix model has A={n_class}")
    if n_out == 1 and n_class != 2:
        raise ValueError("xgboost model: single-output booster for a model with more than 2 ancestries")
    if len(t["tree_class"]) != len(t["tree_off"]) - 1 or (len(t["tree_class"]) and t["tree_class"].max() >= n_out):
        raise ValueError("xgboost model: tree_info does not match the number of classes")
    return {k: t[k] for k in ("tree_off", "left", "right", "feat", "cond", "tree_class", "base_score", "default_left")}


def forest_from_xgb_json(window_dumps, n_class, base_score=0.5, missing=2):
    """Per-window xgboost JSON dumps (XGBBase: one XGBClassifier per window, src/Base/models.py:24-35) -> the fb_*
    arrays of GnxModelData.  multi:softprob lays trees out round-major (tree t -> class t % A); binary:logistic
    (A == 2) has one tree per round."""
    per_round = 1 if n_class == 2 else n_class
    parts = [trees_from_xgb_json(dumps, per_round, base_score) for dumps in window_dumps]
    return forest_from_parts(parts, missing=missing)


def forest_from_parts(parts, missing=2):
    """per-window xgboost-schema dicts (trees_from_xgb_json / refpickle.parse_xgb_raw) -> the fb_* arrays"""
    base_score = parts[0]["base_score"] if parts else 0.5
    wt0 = np.concatenate([[0], np.cumsum([len(p["tree_off"]) - 1 for p in parts])]).astype(np.int32)
    node0 = np.concatenate([[0], np.cumsum([p["tree_off"][-1] for p in parts])])
    return dict(fb_win_tree0=wt0,
                fb_tree_off=np.concatenate([p["tree_off"][:-1] + node0[i] for i, p in enumerate(parts)]
                                           + [[node0[-1]]]).astype(np.int32),
                fb_left=np.concatenate([p["left"] for p in parts]), fb_right=np.concatenate([p["right"] for p in parts]),
                fb_feat=np.concatenate([p["feat"] for p in parts]), fb_cond=np.concatenate([p["cond"] for p in parts]),
                fb_default_left=np.concatenate([p["default_left"] for p in parts]),
                fb_tree_class=np.concatenate([p["tree_class"] for p in parts]),
                fb_base_score=float(base_score), fb_missing=int(missing))


def _int_threshold_as_less_than(thr):
    """SNPs only take the values 0..3, the forest loader asks `x < cond` (xgboost): `x <= thr` of LightGBM / CatBoost is
    `x < floor(thr) + 1` on integers, and floor(thr) + 1 is exact in float32 wherever it matters (clamped to [-1, 5])"""
    return np.float32(min(max(np.floor(float(thr)) + 1.0, -1.0), 5.0))


def _fold_two_outputs(d):
    """A two-output softmax model (LightGBM multiclass with num_class=2, CatBoost MultiClass on two labels) for a two-ancestry
    Gnomix model: the forest kernels treat A == 2 as ONE margin through a sigmoid (xgboost's binary:logistic, k_base_forest.hip),
    and softmax([m0, m1])[1] = sigmoid(m1 - m0) — so class 0's trees enter with their leaves negated and every tree feeds the one
    margin."""
    leaf = d["left"] < 0
    cls_of_node = np.repeat(d["tree_class"], np.diff(d["tree_off"]))
    cond = d["cond"].copy()
    cond[leaf & (cls_of_node == 0)] *= np.float32(-1.0)
    d["cond"] = cond
    d["tree_class"] = np.zeros_like(d["tree_class"])
    return d


def trees_from_lgbm_text(model_str, n_class, missing=2):
    """A LightGBM model string (Booster.model_to_string(), the `handle` a pickled LGBMClassifier's booster carries) ->
    xgboost-schema arrays for the forest base (LGBMBase, src/Base/models.py:38-52: 20 rounds, max_depth 4).

    LightGBM's text format, per tree: `num_leaves`, and for the num_leaves - 1 internal nodes `split_feature`, `threshold`,
    `decision_type`, `left_child`, `right_child` (a child >= 0 is an internal node, a child < 0 is leaf ~child), then `leaf_value`
    per leaf; a numerical node sends `x <= threshold` LEFT.  decision_type: bit 0 categorical, bit 1 default-left, bits 2-3 the
    missing type (0 none, 1 zero, 2 NaN).  The reference feeds int8 SNPs with the missing code 2 as an ordinary number (its own
    comment: "use np.nan for missing encoding" — it does not), so value 2 simply compares: default direction = (2 <= threshold).
    Multiclass: tree t adds to class t % num_tree_per_iteration, probabilities = softmax of the sums (the constant xgboost's
    base_score adds to every class cancels); binary: ONE tree per round, P(class 1) = sigmoid(sigmoid_param * sum).
    The first round's leaves already contain the initial score (boost_from_average)."""
    head, *blocks = model_str.split("\nTree=")
    hp = dict(l.split("=", 1) for l in head.splitlines() if "=" in l)
    per_iter = int(hp.get("num_tree_per_iteration", 1))
    n_out = int(hp.get("num_class", 1))
    if n_out > 1 and n_out != n_class:
        raise ValueError(f"LightGBM model: num_class={n_out} but the Gnomix model has A={n_class}")
    if n_out == 1 and n_class != 2:
        raise ValueError("LightGBM model: single-output booster for a model with more than 2 ancestries")
    if "average_output" in head.split():
        raise NotImplementedError("LightGBM model: average_output (boosting=rf) averages its trees instead of summing them")
    obj = hp.get("objective", "")
    if n_out > 1 and obj.split()[:1] == ["multiclassova"]:
        raise NotImplementedError("LightGBM model: multiclassova (per-class sigmoids, not a softmax)")
    scale = 1.0
    if n_out == 1:
        for tok in obj.split():
            if tok.startswith("sigmoid:"):
                scale = float(tok.split(":", 1)[1])
    off, L, R, F, Cd, Dl, cls = [0], [], [], [], [], [], []
    for t, blk in enumerate(blocks):
        body = blk.split("end of trees")[0]
        kv = dict(l.split("=", 1) for l in body.splitlines() if "=" in l)
        nl = int(kv["num_leaves"])
        if int(kv.get("num_cat", 0)) != 0:
            raise NotImplementedError("LightGBM model: categorical splits (SNPs are numerical features)")
        if int(kv.get("is_linear", 0)) != 0:
            raise NotImplementedError("LightGBM model: linear trees")
        lv = [float(x) for x in kv["leaf_value"].split()]
        if nl == 1:
            L.append(-1); R.append(-1); F.append(0); Cd.append(np.float32(lv[0] * scale)); Dl.append(0)
        else:
            sf = [int(x) for x in kv["split_feature"].split()]
            th = [float(x) for x in kv["threshold"].split()]
            dt = [int(x) for x in kv["decision_type"].split()]
            lc = [int(x) for x in kv["left_child"].split()]
            rc = [int(x) for x in kv["right_child"].split()]
            if not (len(sf) == len(th) == len(dt) == len(lc) == len(rc) == nl - 1 and len(lv) == nl):
                raise ValueError(f"LightGBM model: tree {t} has inconsistent array lengths")
            # node ids of this tree: internal node i -> i, leaf j -> (nl - 1) + j; the root is internal node 0
            nid = lambda c: c if c >= 0 else (nl - 1) + (~c)
            for i in range(nl - 1):
                if dt[i] & 1:
                    raise NotImplementedError("LightGBM model: categorical split")
                if (dt[i] >> 2) & 3 == 1:
                    raise NotImplementedError("LightGBM model: zero_as_missing splits (value 0 would take the default direction)")
                L.append(nid(lc[i])); R.append(nid(rc[i])); F.append(sf[i]); Cd.append(_int_threshold_as_less_than(th[i]))
                Dl.append(int(float(missing) <= th[i]))
            for j in range(nl):
                L.append(-1); R.append(-1); F.append(0); Cd.append(np.float32(lv[j] * scale)); Dl.append(0)
        off.append(len(L))
        cls.append(t % per_iter if n_out > 1 else 0)
    d = dict(tree_off=np.array(off, np.int32), left=np.array(L, np.int32), right=np.array(R, np.int32),
             feat=np.array(F, np.int32), cond=np.array(Cd, np.float32), tree_class=np.array(cls, np.int32),
             base_score=0.5, default_left=np.array(Dl, np.uint8))
    return _fold_two_outputs(d) if n_out == 2 else d


def forest_from_lgbm_text(window_model_strs, n_class, missing=2):
    """Per-window LightGBM model strings (LGBMBase: one LGBMClassifier per window) -> the fb_* arrays of GnxModelData"""
    return forest_from_parts([trees_from_lgbm_text(s, n_class, missing) for s in window_model_strs], missing=missing)


def lgbm_text_of(lgbm_obj):
    """the model string of a fitted LGBMClassifier: from the live booster, or from the attribute bag a stubbed pickle carries
    (lightgbm.Booster.__getstate__ replaces the native handle by model_to_string())"""
    b = getattr(lgbm_obj, "_Booster", None) or getattr(lgbm_obj, "booster_", None)
    if b is None:
        raise ValueError("LGBMClassifier without a fitted booster")
    if hasattr(b, "model_to_string"):
        return b.model_to_string()
    h = getattr(b, "handle", None) or getattr(b, "_handle", None)
    if isinstance(h, bytes):
        h = h.decode()
    if not isinstance(h, str):
        raise ValueError("pickled LightGBM booster without its model string")
    return h


def trees_from_catboost_json(model, n_class, missing=2):
    """A CatBoost model exported with save_model(..., format="json") (dict or str) -> xgboost-schema arrays for the forest base
    (CBBase, src/Base/models.py:68-81: 20 oblivious trees of depth 4).

    An oblivious tree is a list of `splits` (float_feature_index, border) — the SAME split for every node of a level — and
    2^depth leaves; the leaf index has bit i set iff x[feature_i] > border_i.  MultiClass: leaf_values holds n_class numbers per
    leaf (leaf-major), raw_c = scale * sum over trees + bias_c, probabilities = softmax; Logloss (two classes): one number per leaf,
    P(class 1) = sigmoid(raw).  Every oblivious tree becomes one complete binary tree per class (split depth-1 at the root: the
    index's most significant bit first), `x > border` = right; the bias goes into the class's first tree."""
    m = json.loads(model) if isinstance(model, str) else model
    ot = m["oblivious_trees"]
    sb = m.get("scale_and_bias", [1.0, [0.0]])
    scale = float(sb[0])
    bias = sb[1] if isinstance(sb[1], (list, tuple)) else [sb[1]]
    dims = 1
    if ot:
        dims = max(1, len(ot[0]["leaf_values"]) >> len(ot[0].get("splits", [])))
    if dims > 1 and dims != n_class:
        raise ValueError(f"CatBoost model: {dims} output dimensions but the Gnomix model has A={n_class}")
    if dims == 1 and n_class != 2:
        raise ValueError("CatBoost model: single-output model for a model with more than 2 ancestries")
    bias = [float(b) for b in bias] + [0.0] * max(0, dims - len(bias))
    off, L, R, F, Cd, Dl, cls = [0], [], [], [], [], [], []
    for t, tree in enumerate(ot):
        splits = tree.get("splits", [])
        d = len(splits)
        for sp in splits:
            if sp.get("split_type", "FloatFeature") != "FloatFeature":
                raise NotImplementedError("CatBoost model: only float-feature splits (SNPs are numerical features)")
        lv = tree["leaf_values"]
        if len(lv) != (dims << d):
            raise ValueError(f"CatBoost model: tree {t} has {len(lv)} leaf values for depth {d}")
        for c in range(dims):
            base = len(L)
            n_int = (1 << d) - 1
            # heap order inside the tree: internal node h (0-based) at level l tests split d-1-l; children 2h+1, 2h+2
            for h in range(n_int):
                lvl = (h + 1).bit_length() - 1
                sp = splits[d - 1 - lvl]
                L.append(2 * h + 1); R.append(2 * h + 2); F.append(int(sp["float_feature_index"]))
                Cd.append(_int_threshold_as_less_than(sp["border"]))
                Dl.append(int(float(missing) <= float(sp["border"])))
            for leaf in range(1 << d):   # heap leaf order = index with the root's bit as the most significant one
                v = scale * float(lv[leaf * dims + c]) + (bias[c] if t == 0 else 0.0)
                L.append(-1); R.append(-1); F.append(0); Cd.append(np.float32(v)); Dl.append(0)
            assert len(L) - base == n_int + (1 << d)
            off.append(len(L))
            cls.append(c)
    d = dict(tree_off=np.array(off, np.int32), left=np.array(L, np.int32), right=np.array(R, np.int32),
             feat=np.array(F, np.int32), cond=np.array(Cd, np.float32), tree_class=np.array(cls, np.int32),
             base_score=0.5, default_left=np.array(Dl, np.uint8))
    return _fold_two_outputs(d) if dims == 2 else d


def forest_from_catboost_json(window_models, n_class, missing=2):
    """Per-window CatBoost JSON exports (CBBase: one CatBoostClassifier per window) -> the fb_* arrays of GnxModelData"""
    return forest_from_parts([trees_from_catboost_json(m, n_class, missing) for m in window_models], missing=missing)


class _TreeView:
    """sklearn.tree._tree.Tree, real or as the attribute bag a stubbed pickle carries (Tree.__getstate__: `nodes` is a
    structured array with left_child / right_child / feature / threshold, `values` the (n_nodes, n_outputs, n_classes) array)"""

    def __init__(self, t):
        if hasattr(t, "children_left"):
            self.children_left, self.children_right = np.asarray(t.children_left), np.asarray(t.children_right)
            self.feature, self.threshold, self.value = np.asarray(t.feature), np.asarray(t.threshold), np.asarray(t.value)
        else:
            nodes = t.nodes
            self.children_left, self.children_right = np.asarray(nodes["left_child"]), np.asarray(nodes["right_child"])
            self.feature, self.threshold, self.value = np.asarray(nodes["feature"]), np.asarray(nodes["threshold"]), np.asarray(t.values)
        self.node_count = len(self.children_left)


def rforest_from_sklearn(models, n_class):
    """Per-window fitted sklearn RandomForestClassifier (RFBase, src/Base/models.py:54-66) -> the rf_* arrays.
    rf_value[node] is what DecisionTreeClassifier.predict_proba returns for a sample that ends in `node`: tree_.value's
    row, divided by its sum on the scikit-learn versions whose predict_proba still normalises (counts in tree_.value)."""
    import inspect
    from sklearn.tree import DecisionTreeClassifier
    normalise = "normalizer" in inspect.getsource(DecisionTreeClassifier.predict_proba)
    # (a stubbed pickle of an older scikit-learn carries class COUNTS in tree_.value: rows that do not sum to 1 are
    # normalised below exactly as that version's predict_proba did)
    wt0, off, L, R, F, T, V = [0], [0], [], [], [], [], []
    for i, m in enumerate(models):
        if list(m.classes_) != list(range(n_class)):
            raise ValueError(f"window {i}: classes_ != 0..A-1 (the vectorized reference path has no remap, base.py:176)")
        for e in m.estimators_:
            t = _TreeView(e.tree_)
            proba = np.array(t.value[:, 0, :n_class], dtype=np.float64)
            if normalise or not np.allclose(proba.sum(axis=1), 1.0, atol=1e-9):
                normalizer = proba.sum(axis=1)[:, np.newaxis]
                normalizer[normalizer == 0.0] = 1.0
                proba /= normalizer
            L.append(np.asarray(t.children_left, np.int32)); R.append(np.asarray(t.children_right, np.int32))
            F.append(np.where(t.children_left == -1, 0, t.feature).astype(np.int32))
            T.append(np.asarray(t.threshold, np.float64)); V.append(proba)
            off.append(off[-1] + t.node_count)
        wt0.append(len(off) - 1)
    return dict(rf_win_tree0=np.array(wt0, np.int32), rf_tree_off=np.array(off, np.int32), rf_left=np.concatenate(L),
                rf_right=np.concatenate(R), rf_feat=np.concatenate(F), rf_thr=np.concatenate(T), rf_value=np.concatenate(V))


def calibrator_arrays(iso_models):
    """fitted sklearn IsotonicRegression per class (Calibration.py:55) -> calib_off / calib_x / calib_y"""
    off, xs, ys = [0], [], []
    for m in iso_models:
        xs.append(np.asarray(m.X_thresholds_, dtype=np.float64))
        ys.append(np.asarray(m.y_thresholds_, dtype=np.float64))
        off.append(off[-1] + len(xs[-1]))
    return dict(calib_off=np.array(off, np.int32), calib_x=np.concatenate(xs), calib_y=np.concatenate(ys),
                calib_is_f32=bool(np.asarray(iso_models[0].X_thresholds_).dtype == np.float32))


def lr_rows_from_sklearn(coef_, intercept_, n_class):
    """coef_ / intercept_ of one fitted LogisticRegression(solver="liblinear") -> the (A, width) / (A,) rows of the
    one-vs-rest form the kernel evaluates, P_a = expit(z_a) / sum_b expit(z_b).
    A >= 3: sklearn's `_predict_proba_lr` is exactly that form, the arrays pass through.
    A == 2: sklearn keeps ONE row (coef_ (1, n), intercept_ (1,)) and returns [1 - expit(z), expit(z)]; since
    1 - expit(z) = expit(-z) and expit(-z) + expit(z) = 1 the same probabilities are the OvR form of the two rows
    (-coef_, +coef_) / (-b, +b) — copying the single row into both classes would give 0.5 / 0.5 everywhere."""
    coef = np.asarray(coef_, dtype=np.float64)
    icpt = np.asarray(intercept_, dtype=np.float64).reshape(-1)
    if coef.ndim != 2:
        raise ValueError("coef_ must be 2-D")
    if n_class == 2 and coef.shape[0] == 1:
        return np.concatenate([-coef, coef], axis=0), np.array([-icpt[0], icpt[0]])
    if coef.shape[0] != n_class or icpt.shape[0] != n_class:
        raise ValueError(f"coef_ has {coef.shape[0]} rows for {n_class} classes")
    return coef, icpt


def from_reference_model(model) -> GnxModelData:
    """An unpickled reference `src.model.Gnomix` -> GnxModelData."""
    C, M, A = int(model.C), int(model.M), int(model.A)
    d = GnxModelData(C=C, M=M, A=A, S=int(model.smooth.S), context=int(model.context))
    W = C // M
    models = model.base.models
    first = type(models[0]).__name__
    if first == "LogisticRegression":
        ldc = d.M_ + d.rem
        d.base_kind = "logistic"
        d.lr_coef = np.zeros((W, A, ldc))
        d.lr_intercept = np.zeros((W, A))
        for i, m in enumerate(models):
            if list(m.classes_) != list(range(A)):
                raise ValueError(f"window {i}: classes_ != 0..A-1 (the vectorized reference path has no remap, base.py:176)")
            coef, icpt = lr_rows_from_sklearn(m.coef_, m.intercept_, A)
            d.lr_coef[i, :, :coef.shape[1]] = coef
            d.lr_intercept[i] = icpt
    elif first == "SVC":
        d.base_kind = "covrsk"
        kname = getattr(getattr(model.base, "kernel", None), "__name__", "CovRSK")
        d.svc = [svc_window_from_sklearn(m, d.window_width(i), kname) for i, m in enumerate(models)]
    elif first == "KNeighborsClassifier":  # KNNBase (src/Base/models.py:135-146); the per-window arrays are kept as fitted
        d.base_kind = "knn"
        d.knn = [knn_window_from_sklearn(m, d.window_width(i), A) for i, m in enumerate(models)]
    elif first in NB_KINDS:  # NBBernoulliBase / NBMultinomialBase / NBGaussianBase (src/Base/models.py:96-132) -> likelihood tables
        d.base_kind, d.nb_kind = "nb", NB_KINDS[first]
        d.nb_table = np.zeros((W, d.M_ + d.rem, 4, A))
        d.nb_bias = np.zeros((W, A))
        for i, m in enumerate(models):
            try:
                t, b = nb_window_from_sklearn(m, d.window_width(i), A, kind=d.nb_kind)
            except ValueError as e:
                raise ValueError(f"window {i}: {e}") from e
            d.nb_table[i, :t.shape[0]] = t
            d.nb_bias[i] = b
    elif first == "LinearDiscriminantAnalysis":  # LDABase (src/Base/models.py:83-94): coef_ / intercept_ as fitted
        R = 1 if A == 2 else A
        d.base_kind = "lda"
        d.lda_coef = np.zeros((W, R, d.M_ + d.rem))
        d.lda_intercept = np.zeros((W, R))
        for i, m in enumerate(models):
            try:
                coef, icpt = lda_from_sklearn(m, d.window_width(i), A)
            except ValueError as e:
                raise ValueError(f"window {i}: {e}") from e
            d.lda_coef[i, :, :coef.shape[1]] = coef
            d.lda_intercept[i] = icpt
    elif first == "XGBClassifier":  # XGBBase (src/Base/models.py:24-35)
        d.base_kind = "forest"
        parts = [xgb_trees_of(m, A) for m in models]
        for k, v in forest_from_parts(parts, missing=int(getattr(model.base, "missing_encoding", 2))).items():
            setattr(d, k, v)
    elif first == "LGBMClassifier":  # LGBMBase (src/Base/models.py:38-52): the boosters' own model strings, no lightgbm needed
        d.base_kind = "forest"
        for k, v in forest_from_lgbm_text([lgbm_text_of(m) for m in models], A,
                                          missing=int(getattr(model.base, "missing_encoding", 2))).items():
            setattr(d, k, v)
    elif first == "CatBoostClassifier":  # CBBase (src/Base/models.py:68-81): through CatBoost's JSON export (needs catboost:
        import json as _json              # its pickle carries the binary model blob)
        import os as _os
        import tempfile
        d.base_kind = "forest"
        exports = []
        for m in models:
            if not hasattr(m, "save_model"):
                raise NotImplementedError("CBBase from a stubbed pickle: export every window with save_model(format='json') and use "
                                          "gnomix_amd.convert.forest_from_catboost_json")
            with tempfile.TemporaryDirectory() as td:
                fn = _os.path.join(td, "m.json")
                m.save_model(fn, format="json")
                exports.append(_json.load(open(fn)))
        for k, v in forest_from_catboost_json(exports, A, missing=int(getattr(model.base, "missing_encoding", 2))).items():
            setattr(d, k, v)
    elif first == "RandomForestClassifier":  # RFBase (src/Base/models.py:54-66)
        d.base_kind = "rforest"
        for k, v in rforest_from_sklearn(models, A).items():
            setattr(d, k, v)
    else:
        raise NotImplementedError(f"base model {first}")
    sm = type(model.smooth).__name__
    if sm == "XGB_Smoother":
        t = xgb_trees_of(model.smooth.model, A)
        if A == 2 and len(t["tree_class"]) and t["tree_class"].max() == 0:
            raise NotImplementedError("binary:logistic smoother (A == 2 trained by xgboost's sklearn wrapper)")
        d.smooth_kind = "xgb"
        for k, v in t.items():
            if k != "default_left":  # smoother features are probabilities, never missing
                setattr(d, k, v)
    elif sm == "CRF_Smoother":
        crf = model.smooth.model.CRF
        d.smooth_kind = "crf"
        d.crf_state = np.zeros((A, A))
        d.crf_trans = np.zeros((A, A))
        for (attr, label), w in crf.state_features_.items():
            d.crf_state[int(attr), int(label)] = w
        for (y0, y1), w in crf.transition_features_.items():
            d.crf_trans[int(y0), int(y1)] = w
    elif sm == "CNN_Smoother":  # mode "large" (src/model.py:65-67): src.Smooth.cnn.CNN holds nn.Sequential(nn.Conv1d(A, A, S))
        conv = model.smooth.model.smoothNet[0]
        d.smooth_kind = "cnn"
        d.cnn_weight = np.ascontiguousarray(conv.weight.detach().cpu().numpy(), dtype=np.float32)
        d.cnn_bias = np.ascontiguousarray(conv.bias.detach().cpu().numpy(), dtype=np.float32)
        if d.cnn_weight.shape != (A, A, d.S):
            raise ValueError(f"CNN smoother: Conv1d weight {d.cnn_weight.shape} != (A, A, S) = ({A}, {A}, {d.S})")
    else:
        raise NotImplementedError(f"smoother {sm}")
    cal = getattr(model.smooth, "calibrator", None)
    if cal is not None and all(mm is not None for mm in cal.models):
        for k, v in calibrator_arrays(cal.models).items():
            setattr(d, k, v)
    mf = getattr(model.smooth, "mode_filter", 0)
    if mf:   # (0, False and None all mean "off", src/Smooth/smooth.py:63, utils.py:39)
        d.mode_filter = int(mf)
    d.snp_pos, d.snp_ref, d.snp_alt = model.snp_pos, model.snp_ref, model.snp_alt
    d.population_order = list(model.population_order) if model.population_order is not None else None
    gm = getattr(model, "gen_map_df", None)
    if gm is not None and len(gm):
        d.gen_map_pos, d.gen_map_cm = np.asarray(gm["pos"]), np.asarray(gm["pos_cm"])
    return d
