/*
 * gnomix_hip.h — C ABI of libgnomix_hip.so: the MI355X (gfx950) implementation of the Gnomix
 * inference hot path  X (phased SNPs, int8) -> per-window base classifier -> B -> sliding-window
 * smoother -> per-window ancestry probabilities / labels  (+ the Gnofix re-phasing loop).
 *
 * The reference (AI-sandbox/gnomix, /root/reference) is pure Python and has no FFI of its own; the
 * entry points below are what a binding for this path replaces, one per reference call site:
 *
 *   gnx_model_load        <- pickle.load of src.model.Gnomix            gnomix.py:26-35 (load_model)
 *   gnx_base_predict      <- Base.predict_proba(X)                      src/Base/base.py:129-180, gnomix.py:55
 *   gnx_smooth_predict    <- Smoother.predict_proba(B) / .predict(B)    src/Smooth/smooth.py:40-65, gnomix.py:57-58
 *   gnx_infer             <- Gnomix.predict_proba(X) / .predict(X)      src/model.py:169-179, gnomix.py:72
 *   gnx_smooth_rows       <- smoother.model.predict_proba(rows)         src/Gnofix/gnofix.py:157
 *   gnx_gnofix            <- Gnomix.phase(X, B) -> gnofix() per indiv.  src/model.py:188-214, src/Gnofix/gnofix.py:58-208
 *   gnx_gnofix_ex         <- gnofix(..., check_criterion, max_center_offset, non_lin_s, prob_comp, prior_switch_prob, padding)
 *   gnx_train_logistic    <- Base.train(X, y) of LogisticRegressionBase   src/Base/base.py:104-127, src/model.py:113,155
 *   gnx_train_svc         <- Base.train(X, y) of CovRSKBase (mode "best") src/Base/base.py:104-127, src/Base/models.py:195-215
 *   gnx_train_svc2        <- the same, and Base.train(X, y) of SVMBase (RBF)  src/Base/models.py:148-159
 *                            (gnx_train_svc with GNX_SVC_KERNEL_ALL_LENGTHS: Base.train(X, y) of StringKernelBase, models.py:161-176)
 *   gnx_train_svc_poly    <- Base.train(X, y) of PolynomialStringKernelBase  src/Base/models.py:178-193, string_kernel.py:40-61
 *   gnx_svc_gram          <- the kernel callables themselves on a window's training rows: CovRSK_DP_triangular_numbers(Xw, Xw),
 *                            string_kernel_DP_triangular_numbers(Xw, Xw), poly_kernel(Xw, Xw)   src/Base/string_kernel.py
 *   gnx_train_gbt_base    <- Base.train(X, y) of XGBBase (boosted trees)  src/Base/base.py:104-127, src/Base/models.py:24-35
 *   gnx_train_rforest     <- Base.train(X, y) of RFBase                   src/Base/models.py:54-66
 *   (no entry point)      <- Base.train(X, y) of KNNBase: a 1-NN fit stores its rows; the caller puts them into
 *                            gnx_model_desc.knn and loads the model                src/Base/models.py:135-146
 *   gnx_train_nb_counts   <- Base.train(X, y) of NBBernoulliBase / NBMultinomialBase / NBGaussianBase: the integer counts
 *                            every closed form needs; the caller finishes in float64 and loads the tables through
 *                            gnx_model_load_nb                                     src/Base/models.py:96-132
 *   gnx_train_lda_gram    <- Base.train(X, y) of LDABase: the exact integer Gram matrix, class sums and class counts of every
 *                            window; the caller finishes scikit-learn's svd solver in float64 and loads coef_ / intercept_
 *                            through gnx_model_load_lda                            src/Base/models.py:83-94
 *   gnx_train_gbt         <- Smoother.train(B, y) of XGB_Smoother         src/Smooth/smooth.py:28-38, src/model.py:137
 *   gnx_train_crf         <- Smoother.train(B, y) of CRF_Smoother         src/Smooth/crf.py:51-58, src/Smooth/models.py:27-32
 *   gnx_train_cnn         <- Smoother.train(B, y) of CNN_Smoother         src/Smooth/cnn.py:104-118, src/Smooth/models.py:35-42
 *   gnx_simulate_admix    <- LAIDataset.simulate + write_output + data_process   src/laidataset.py:119-201, 362-428,
 *                                                                          src/preprocess.py:37-82, gnomix.py:102-156
 *   gnx_mode_filter       <- Smoother.predict's mode_filter               src/Smooth/utils.py:31-46, src/Smooth/smooth.py:63-64
 *   gnx_label_runs        <- get_bed_data's walk over a haplotype column  src/postprocess.py:162-193
 *   gnx_ancestry_summary  <- (no counterpart: the .Q table and the tract statistics users compute from an .msp)
 *   gnx_ancestry_allele_counts <- (no counterpart: the join of the labels with the genotypes: ancestry-specific allele counts and dosages)
 *
 * Conventions
 *   - return 0 (GNX_OK) or a negative GNX_E* code; the message is kept per context (gnx_last_error).
 *     No exception or signal crosses this ABI.  (The reference aborts with Python assert/exception:
 *     src/model.py:193-194, src/Smooth/models.py:13, src/Smooth/smooth.py:31 — the Python mirror in
 *     gnomix_amd/ turns the codes back into those exceptions.)
 *   - plain pointers and sizes only; the library never frees or keeps caller memory
 *     (gnx_model_load copies what it needs).
 *   - un-suffixed entry points take HOST pointers, are synchronous and stage through the context's
 *     device workspaces (gnx_infer / gnx_infer_packed in batches, the copy-in of batch i+1, the kernels of
 *     batch i and the copy-out of batch i-1 overlapped on three streams); *_dev entry points take DEVICE pointers (same device as the context), are
 *     asynchronous on the context stream (gnx_set_stream / gnx_synchronize) and never allocate
 *     when the workspace is already large enough.
 *   - one gnx_ctx per device; a context and its models are not thread-safe (the reference is
 *     single-threaded at this level: src/model.py:205); different contexts may live on different
 *     threads or processes (one process per GPU under torch.distributed).
 *   - haplotype rows 2i, 2i+1 of X are the two haplotypes of individual i (src/utils.py:121-123);
 *     X values are {0,1,2=missing} int8, the value 2 enters the logistic model as the number 2
 *     (sklearn sees it as a feature value) and string kernels as a third symbol.  The logistic base takes
 *     ANY int8 value as the signed number it is (exact in the integer kernels while 128 * max|x| * K < 2^31
 *     for windows of K SNPs); 2-bit rows hold 0..3 and gnx_pack_x refuses anything else (GNX_EINVAL).
 *   - a NaN or an infinity in lr_coef (the columns a window uses) or lr_intercept fails gnx_model_load with
 *     GNX_EINVAL; so does a coefficient beyond 1e300.
 */
#ifndef GNOMIX_HIP_H
#define GNOMIX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNX_ABI_VERSION 16

typedef struct gnx_ctx gnx_ctx;
typedef struct gnx_model gnx_model;

enum {
  GNX_OK = 0,
  GNX_EINVAL = -1,       /* bad argument / inconsistent model description */
  GNX_ENOMEM = -2,       /* host or device allocation failed */
  GNX_EHIP = -3,         /* HIP runtime error (message has the hipError string) */
  GNX_EUNSUPPORTED = -4, /* valid in the reference but not built here (message says what) */
  GNX_ESTATE = -5,       /* call not valid for this model (e.g. phasing with a CRF smoother) */
  GNX_ESTALE = -6        /* gnx_model_desc.prepared does not belong to this model / library / settings, or is truncated: nothing was
                            loaded; load again without it (and write a new one) */
};

enum { GNX_SVC_KERNEL_SUBSTRINGS = 0, GNX_SVC_KERNEL_POLY = 1, GNX_SVC_KERNEL_ALL_LENGTHS = 2 /* gnx_train_svc only */,
       GNX_SVC_KERNEL_RBF = 3 /* SVMBase: exp(-gamma |x - y|^2) on the SNP codes as numbers */ };
enum { GNX_BASE_NONE = 0, GNX_BASE_LOGISTIC = 1, GNX_BASE_COVRSK_SVC = 2, GNX_BASE_FOREST = 3, GNX_BASE_RFOREST = 4,
       GNX_BASE_KNN = 5 /* KNNBase: 1-nearest neighbour per window */,
       GNX_BASE_NB = 6 /* the three Naive-Bayes bases: per-window likelihood tables, loaded through gnx_model_load_nb */,
       GNX_BASE_LDA = 7 /* LDABase: per-window linear discriminant, loaded through gnx_model_load_lda */ };
enum { GNX_SMOOTH_NONE = 0, GNX_SMOOTH_XGB = 1, GNX_SMOOTH_CRF = 2, GNX_SMOOTH_CNN = 3 };

/* kernel ids for gnx_profile_get */
enum {
  GNX_K_BASE_LOGISTIC = 0,
  GNX_K_SMOOTH_XGB = 1,
  GNX_K_BASE_COVRSK = 2,
  GNX_K_SMOOTH_CRF = 3,
  GNX_K_GNOFIX = 4,
  GNX_K_SMOOTH_ROWS = 5,
  GNX_K_CALIBRATE = 6,
  GNX_K_BASE_FOREST = 7,
  GNX_K_SMOOTH_CNN = 8,
  GNX_K_COUNT = 9
};

/* Per-window SVC of CovRSKBase (src/Base/models.py:195-215 -> sklearn.svm.SVC(kernel=callable,
 * probability=True)) or of SVMBase (src/Base/models.py:148-159 -> SVC(C=100., gamma=0.001, probability=True), libsvm's RBF
 * kernel); field names follow the fitted sklearn attributes.
 * GNX_SVC_KERNEL_RBF: K(x, y) = exp(-gamma |x - y|^2) with the SNP codes taken as numbers (2 = missing is the number 2, as
 * everywhere in the reference).  xfit rows must hold 0..2 (GNX_EINVAL otherwise), gamma must be finite and > 0, the width at
 * most GNX_RBF_MAX_WIDTH; every window of a model has the same kernel_kind; ms / run_value / poly_p are unused.  |x - y|^2 is
 * an exact integer (int8 matrix cores) and K is read from a table T[k] = exp(-gamma k) that gnx_model_load fills with the
 * host C library's exp, k = 0 .. 9 * width: a QUERY code 3 (the largest a 2-bit packed row can hold) is HANDLED, as the
 * number 3, identically by the int8 and the 2-bit entry points; other int8 query values are outside the contract (the
 * distance is clamped to the table's last entry, nothing is read out of bounds).
 * A model holds at most GNX_RBF_MAX_A ancestries (GNX_EUNSUPPORTED beyond): the limit of the CovRSK base, whose pairwise-coupling
 * pass (multiclass_probability with A(A-1)/2 + A*A + 2A float64 values per haplotype in LDS) the RBF base shares.  gnx_train_svc2
 * itself fits up to 32; what it fits beyond GNX_RBF_MAX_A cannot be loaded for inference by this build. */
#define GNX_RBF_MAX_WIDTH 8192
#define GNX_RBF_MAX_A 13
typedef struct gnx_svc_window {
  const int8_t* xfit;       /* (n_fit, width) training rows, row-major (sklearn __Xfit) */
  int32_t n_fit;
  int32_t width;            /* M_ (or M_+rem for the last window) */
  const int32_t* support;   /* (n_sv,) indices into xfit (support_) */
  int32_t n_sv;
  const double* dual_coef;  /* (A-1, n_sv) (_dual_coef_) */
  const double* intercept;  /* (A(A-1)/2,) (_intercept_ = -rho) */
  const double* prob_a;     /* (A(A-1)/2,) (_probA) */
  const double* prob_b;     /* (A(A-1)/2,) (_probB) */
  const int32_t* n_support; /* (A,) (_n_support) */
  const int32_t* ms;        /* CovSample lengths for this width (string_kernel.py:80-89); unused for GNX_SVC_KERNEL_POLY */
  int32_t n_ms;
  int32_t kernel_kind;      /* GNX_SVC_KERNEL_*: 0 = substring counts over the lengths `ms` (CovRSK; every length = the plain
                               string kernel), 1 = polynomial string kernel (string_kernel.py:40-61) */
  double poly_p;            /* POLY: K = int(np.sum(run_value[run lengths]) / poly_p), p = 1.2 in the reference */
  const double* run_value;  /* POLY: (width+1,) value of a run of L equal SNPs = L ** p as numpy computed it */
  double gamma;             /* RBF: sklearn's _gamma */
} gnx_svc_window;

/* Per-window 1-nearest-neighbour classifier of KNNBase (src/Base/models.py:135-146 -> sklearn
 * KNeighborsClassifier(n_neighbors=1): uniform weights, Euclidean metric).  B[n, w, c] = 1 if c is the label of the fit row
 * nearest to the query's window slice, else 0 (float32 and float64 outputs hold exactly 0 and 1; a class absent from a
 * window's labels gets a zero column).  The squared distance is an exact integer over the SNP codes as numbers (2 = missing is
 * the number 2; a QUERY code 3, the largest a 2-bit packed row can hold, is the number 3, identically through the int8 and the
 * 2-bit entry points).  TIES GO TO THE LOWEST FIT-ROW INDEX: a rule of this library and a deviation, since scikit-learn's
 * choice among equidistant neighbours is unspecified (it depends on the algorithm it resolves to); the outputs agree wherever
 * the minimum-distance rows carry one label.
 * GNX_EINVAL: a code outside 0..2 in xfit, a label outside [0, A), n_fit < 1, width != the window's width.
 * GNX_EUNSUPPORTED: windows wider than GNX_RBF_MAX_WIDTH SNPs. */
typedef struct gnx_knn_window {
  const int8_t* xfit;  /* (n_fit, width) fit rows, row-major, codes 0..2 (sklearn _fit_X) */
  const int32_t* y;    /* (n_fit,) labels in [0, A) (classes_[_y]) */
  int32_t n_fit;       /* >= 1 */
  int32_t width;       /* M_ (or M_+rem for the last window), <= GNX_RBF_MAX_WIDTH */
} gnx_knn_window;

/* Per-window Naive-Bayes classifier of NBBernoulliBase / NBMultinomialBase / NBGaussianBase (src/Base/models.py:96-132 -> sklearn
 * BernoulliNB(alpha=0) / MultinomialNB(alpha=0) / GaussianNB()).  On SNP codes x in {0, 1, 2, 3} all three have one form:
 *   jll[n, c] = bias[c] + sum_p table[p, x[n, col(p)], c]     p = 0 .. width-1 in this order, col = the window's slice of the
 *   B[n, w, :] = softmax_c(jll)                                reflect-padded query (base.py:41-44, 146-164)
 * The sum is a plain sequential float64 sum that starts at bias[c]: one rounding per position, in position order (the kernel adds
 * each table row with one v_mfma_f64_16x16x4_f64 whose other three products are exact zeros).
 * Normalisation: m = max_c jll over the present classes; e_c = exp(jll_c - m); B_c = e_c / sum(e) (one reciprocal per row).
 * The float32 output is the float32 rounding of the float64 output.
 * Table construction is the caller's (gnomix_amd.convert.nb_window_from_sklearn), class column c = classes_[k]:
 *   Bernoulli   (binarize = 0):  table[p,0,c] = log(1 - exp(flp[c,p])), table[p,v>=1,c] = flp[c,p];  bias = class_log_prior_
 *   Multinomial:                 table[p,v,c] = v * flp[c,p];                                        bias = class_log_prior_
 *   Gaussian:                    table[p,v,c] = -0.5 (v - theta_[c,p])^2 / var_[c,p];
 *                                bias[c] = log(class_prior_[c]) - 0.5 sum_p log(2 pi var_[c,p])
 *   (flp = feature_log_prob_.)
 * Codes are numbers: 2 = missing is the number 2; a query code 3 (the largest a 2-bit packed row can hold) reads table row 3, which
 * is the number 3 for Multinomial and Gaussian and "non-zero" for Bernoulli.  Other int8 values are outside the contract: the kernel
 * uses their two low bits, so nothing is read out of bounds.
 * A class absent from a window has bias = -inf: its table rows are ignored (taken as zero) and its output column is exactly 0.
 * -inf is allowed only in bias; at least one class per window must be present.
 * GNX_EINVAL: a non-finite table entry (the message names the window), NaN or +inf in bias, a window with no class present,
 *   width != the window's width, a NULL pointer.  GNX_EUNSUPPORTED: A > 16 (the class columns are one 16-wide MFMA tile). */
typedef struct gnx_nb_window {
  const double* table;  /* (width, 4, A) row-major: [position][code][class], finite */
  const double* bias;   /* (A,) finite, or -inf for a class absent from the window */
  int32_t width;        /* M_ (or M_+rem for the last window) */
  int32_t reserved;
} gnx_nb_window;

/* Per-window linear discriminant of LDABase (src/Base/models.py -> sklearn LinearDiscriminantAnalysis(), solver "svd").  On the
 * window's slice x of the reflect-padded query, the SNP codes as numbers (2 = missing is the number 2):
 *   d[n, r] = sum_p coef[r, p] * x[n, col(p)] + intercept[r]       r = 0 .. n_rows - 1
 *   A > 2:   n_rows = A, B[n, w, :] = softmax_r(d)     (row maximum subtracted; one reciprocal per row)
 *   A == 2:  n_rows = 1 (scikit-learn keeps coef_[1] - coef_[0]);  p = 1 / (1 + exp(-d));  B[n, w, :] = [1 - p, p]
 * The sum runs in float64 on v_mfma_f64_16x16x4_f64 with coef as the float64 it is (nothing is quantised); the order of the
 * additions is the instruction's, so d differs from a numpy evaluation by at most (width + 2) 2^-53 (sum_p |coef x| + |intercept|).
 * The float32 output is the float32 rounding of the float64 output.
 * GNX_EINVAL: a non-finite coefficient or intercept (the message names the window), width != the window's width, n_rows != A
 *   (1 for A == 2), a NULL pointer.  GNX_EUNSUPPORTED: A > 16 (the decision columns are one 16-wide MFMA tile). */
typedef struct gnx_lda_window {
  const double* coef;       /* (n_rows, width) row-major, finite */
  const double* intercept;  /* (n_rows,) finite */
  int32_t width;            /* M_ (or M_+rem for the last window) */
  int32_t n_rows;           /* A, or 1 when A == 2 */
} gnx_lda_window;

/* Everything a pickled src.model.Gnomix carries for inference (src/model.py:28-88), as flat host
 * arrays.  W = C / M (src/model.py:32); the reference requires C % M != 0 (gnomix.py:124-125). */
typedef struct gnx_model_desc {
  int32_t abi_version; /* GNX_ABI_VERSION */
  int32_t A;           /* ancestries */
  int64_t C;           /* SNPs */
  int64_t M;           /* window size in SNPs */
  int64_t ctx;         /* context SNPs each side = int(M*context_ratio) (src/model.py:47) */
  int32_t S;           /* smoother width in windows, odd (src/Smooth/smooth.py:14) */
  int32_t base_kind;   /* GNX_BASE_* */
  int32_t smooth_kind; /* GNX_SMOOTH_* */
  int32_t reserved0;

  /* GNX_BASE_LOGISTIC: LogisticRegression(solver=liblinear) per window, OvR (models.py:12-21) */
  const double* lr_coef;      /* (W, A, lr_ldc): coef_ of window i in [i][a][0:width_i], rest ignored */
  int64_t lr_ldc;             /* >= M + 2ctx + rem */
  const double* lr_intercept; /* (W, A) */

  /* GNX_BASE_COVRSK_SVC */
  const gnx_svc_window* svc;  /* (W,) */

  /* GNX_SMOOTH_XGB: xgboost model schema, node arrays of all trees concatenated
   * (src/Smooth/models.py:14-20: multi:softprob, tree t belongs to class tree_class[t]) */
  int32_t n_trees;
  int32_t n_nodes;           /* length of left/right/feat/cond (0 = not given: tree_off[n_trees] is trusted) */
  const int32_t* tree_off;   /* (n_trees+1,) node offsets: 0, strictly increasing, tree_off[n_trees] == n_nodes */
  const int32_t* left;       /* child index within the tree, -1 at leaves */
  const int32_t* right;
  const int32_t* feat;       /* split feature = s*A + a of the (S*A)-wide sliding window */
  const float* cond;         /* split condition (go left iff f < cond); leaf value at leaves */
  const int32_t* tree_class; /* (n_trees,) */
  float base_score;          /* 0.5 */
  int32_t reserved2;

  /* GNX_SMOOTH_CRF: linear-chain CRF (src/Smooth/crf.py:9-15) */
  const double* crf_state;   /* (A, A) [attribute a][label y] */
  const double* crf_trans;   /* (A, A) [from y'][to y] */

  /* optional Calibrator (src/Smooth/Calibration.py:19-69): per class c the fitted IsotonicRegression's
   * X_thresholds_ / y_thresholds_ in [calib_off[c], calib_off[c+1]); NULL = no calibrator trained */
  const int32_t* calib_off;  /* (A+1,) */
  const double* calib_x;
  const double* calib_y;
  int32_t calib_is_f32;      /* the isotonic maps were fitted on float32 probabilities (the xgb and CNN smoothers' output): sklearn then
                                casts its input to float32 and interpolates in float32, and so does the kernel, narrowing float64
                                inputs first; maps fitted in float64 are evaluated in float64 by np.interp's rules (float32 inputs
                                widened, a value exactly on a threshold returns that threshold's y) */
  int32_t reserved3;

  /* GNX_BASE_FOREST: one gradient-boosted tree ensemble per window (XGBBase, src/Base/models.py:24-35:
   * XGBClassifier(n_estimators=20, max_depth=4, missing=missing_encoding)); xgboost model schema, all windows'
   * trees concatenated.  A >= 3: multi:softprob, tree t adds to class fb_tree_class[t]; A == 2: binary:logistic
   * (every tree adds to the one margin, fb_tree_class ignored).  Split features are SNP indices WITHIN the
   * window's padded slice [i*M, i*M + width_i).  A SNP equal to fb_missing follows fb_default_left. */
  int32_t fb_n_trees;
  int32_t fb_missing;               /* missing_encoding, 2 (src/Base/base.py:25) */
  const int32_t* fb_win_tree0;      /* (W+1,) first tree of each window */
  const int32_t* fb_tree_off;       /* (fb_n_trees+1,) node offsets */
  const int32_t* fb_left;           /* child index within the tree, -1 at leaves */
  const int32_t* fb_right;
  const int32_t* fb_feat;
  const float* fb_cond;             /* split condition (left iff x < cond); leaf value at leaves */
  const uint8_t* fb_default_left;   /* per node: 1 = missing goes left */
  const int32_t* fb_tree_class;     /* (fb_n_trees,) */
  float fb_base_score;              /* 0.5 */
  int32_t fb_n_nodes;               /* length of the fb_ node arrays (0 = not given) */

  /* GNX_BASE_RFOREST: one random forest per window (RFBase, src/Base/models.py:54-66:
   * RandomForestClassifier(n_estimators=20, max_depth=4)); sklearn's tree arrays (tree_.children_left/right, feature,
   * threshold) of all trees of all windows concatenated.  Left iff float32(x) <= threshold; a leaf contributes its
   * class-probability row rf_value[node]; the window's output is the mean over its trees (float64). */
  int32_t rf_n_trees;
  int32_t rf_n_nodes;               /* length of the rf_ node arrays (0 = not given) */
  const int32_t* rf_win_tree0;      /* (W+1,) */
  const int32_t* rf_tree_off;       /* (rf_n_trees+1,) node offsets */
  const int32_t* rf_left;           /* -1 at leaves */
  const int32_t* rf_right;
  const int32_t* rf_feat;           /* SNP index within the window's padded slice */
  const double* rf_thr;
  const double* rf_value;           /* (n_nodes, A) what DecisionTreeClassifier.predict_proba returns at that node */

  /* GNX_SMOOTH_CNN: the "large" mode's smoother (src/Smooth/cnn.py:37-55): one Conv1d(A, A, kernel_size=S,
   * padding=(S-1)/2, zero padding — see k_smooth_cnn.hip) over the windows + softmax over the A output channels */
  const float* cnn_weight;          /* (A_out, A_in, S) smoothNet[0].weight */
  const float* cnn_bias;            /* (A_out,) smoothNet[0].bias */

  /* optional: the logistic base's PREPARED digit planes as gnx_model_export_prepared wrote them for this very model (a command line
   * that loads the same model.pkl / .gnx on every start keeps them in a file beside it: preparing the planes is most of what
   * gnx_model_load does).  Checked against a hash of lr_coef, the geometry, the ABI version and the plane settings; anything that
   * does not match -> GNX_ESTALE, nothing loaded.  NULL / 0: prepare from lr_coef. */
  const void* prepared;
  int64_t prepared_bytes;

  /* GNX_BASE_KNN */
  const gnx_knn_window* knn;  /* (W,) */
} gnx_model_desc;

typedef struct gnx_model_info {
  int64_t C, M, ctx, W;
  int32_t A, S, base_kind, smooth_kind;
  int32_t n_trees, tree_depth;
  int64_t device_bytes; /* HBM held by the model */
} gnx_model_info;

int gnx_abi_version(void);
/* how the library was built: no build variants at present; bits reserved (always 0) */
int gnx_build_flags(void);
/* GPUs this process sees (HIP_VISIBLE_DEVICES applied); 0 without a usable runtime.  One gnx_ctx per device: gnx_init(d), 0 <= d < count. */
int gnx_device_count(void);

/* context */
int gnx_init(int device, gnx_ctx** out);
void gnx_ctx_free(gnx_ctx* ctx);
const char* gnx_last_error(const gnx_ctx* ctx);
int gnx_set_stream(gnx_ctx* ctx, void* hip_stream); /* borrow a hipStream_t; NULL is HIP's default (null) stream */
int gnx_reset_stream(gnx_ctx* ctx);                 /* back to the context's own non-blocking stream */
int gnx_synchronize(gnx_ctx* ctx);
/* page-locked host memory for the host-pointer entry points: buffers allocated here move over PCIe by DMA at link rate
 * (pageable memory goes through the runtime's staging copies).  The reference hands over numpy arrays (gnomix.py:48-49):
 * a caller that lets its VCF reader fill a buffer from gnx_host_alloc avoids that extra pass. */
int gnx_host_alloc(gnx_ctx* ctx, size_t bytes, void** out);
int gnx_host_free(gnx_ctx* ctx, void* p);
/* allocation flags of a gnx_host_alloc buffer (hipHostGetFlags).  Every buffer is hipHostMallocPortable (bit 0): page-locked for
 * EVERY device of the process, because the one-process multi-GPU file path (gnomix_amd/multi.py) hands the same parsed genotype
 * rows and output arrays to contexts on different devices. */
#define GNX_HOST_PORTABLE 0x1u
int gnx_host_flags(const void* p, unsigned* flags);
/* Device binding.  HIP's "current device" belongs to the calling THREAD (a new thread starts on device 0); every entry point of this
 * library that touches the GPU binds its context's device for the duration of the call and restores the caller's on return, so
 * several contexts may be driven from one thread (torch tensors on several GPUs) as well as one context per thread.
 * Diagnostics for that contract: the device ordinal (hipPointerGetAttributes) of every LIVE device workspace of the context, at most
 * n of them written to out; returns how many workspaces are live (may exceed n), negative on error.  A tripwire for multi-GPU
 * nodes: every entry must equal the device the context was created on (tests/test_gpu_devices.py). */
int gnx_debug_ws_devices(gnx_ctx* ctx, int32_t* out, int32_t n);

/* model */
int gnx_model_load(gnx_ctx* ctx, const gnx_model_desc* desc, gnx_model** out);
/* A model whose base is GNX_BASE_NB: desc->base_kind must be GNX_BASE_NB, nb lists the W windows' tables (gnx_nb_window above);
 * everything else in desc (geometry, smoother, calibrator) means what it means to gnx_model_load.  gnx_model_load itself answers
 * GNX_EINVAL to GNX_BASE_NB and names this entry: gnx_model_desc has no field for the tables. */
int gnx_model_load_nb(gnx_ctx* ctx, const gnx_model_desc* desc, const gnx_nb_window* nb /* (W,) */, gnx_model** out);
/* A model whose base is GNX_BASE_LDA: desc->base_kind must be GNX_BASE_LDA, lda lists the W windows' coefficients (gnx_lda_window
 * above); the rest of desc means what it means to gnx_model_load, which itself answers GNX_EINVAL to GNX_BASE_LDA and names this
 * entry. */
int gnx_model_load_lda(gnx_ctx* ctx, const gnx_model_desc* desc, const gnx_lda_window* lda /* (W,) */, gnx_model** out);
void gnx_model_free(gnx_model* model);
int gnx_model_get_info(const gnx_model* model, gnx_model_info* out);
/* smooth.calibrate (gnomix.py:367): when on AND the model carries a calibrator, smoother outputs (probabilities and the
 * labels derived from them) go through Calibrator.transform; without a calibrator the reference prints a notice and
 * returns the original probabilities (smooth.py:48-52) — so does this (GNX_OK, outputs unchanged). */
int gnx_model_set_calibrate(gnx_model* model, int on);
/* the prepared planes of a loaded logistic model as one relocatable blob for gnx_model_desc.prepared: *bytes = its size (0 for models
 * without a logistic base); buf == NULL only reports the size; cap < size -> GNX_EINVAL. */
int gnx_model_export_prepared(gnx_model* model, void* buf, int64_t cap, int64_t* bytes);

/* Base.predict_proba: X (N, ldx>=C) int8 -> B (N, W, A).  Either output may be NULL.
 * b_f32 is what the XGB smoother consumes (src/Smooth/utils.py:20), b_f64 what the reference returns. */
int gnx_base_predict(gnx_model* model, const int8_t* X, int64_t N, int64_t ldx, float* b_f32, double* b_f64);
int gnx_base_predict_dev(gnx_model* model, const int8_t* dX, int64_t N, int64_t ldx, float* d_b_f32, double* d_b_f64);
/* The logistic pass with the rank image gnx_infer_dev hands the tree smoother in place of B (tests): d_rk16 holds
 * ceil(N / 32) * 32 * W * A uint16, [n / 32][w][a][n % 32] = the rank of the float32 probability in the smoother's threshold
 * table (NaN: 0xFFFF); positions of haplotypes >= N are not written.  d_b_f32 may be NULL.  GNX_EUNSUPPORTED for models whose
 * base pass writes no ranks (any base but the int8 logistic pass of one column tile, any smoother without a rank table). */
int gnx_base_predict_ranks_dev(gnx_model* model, const int8_t* dX, int64_t N, int64_t ldx, float* d_b_f32, uint16_t* d_rk16);

/* Smoother.predict_proba / predict: B (N, W, A) (float64 if b_is_f64 else float32) ->
 * proba (N, W, A) and labels (N, W) (argmax, first max wins).  Any output may be NULL.
 * XGB computes in float32 (proba_f64 is the widened copy); CRF computes in float64. */
int gnx_smooth_predict(gnx_model* model, const void* B, int b_is_f64, int64_t N, float* proba_f32,
                       double* proba_f64, int32_t* labels);
int gnx_smooth_predict_dev(gnx_model* model, const void* dB, int b_is_f64, int64_t N, float* d_proba_f32,
                           double* d_proba_f64, int32_t* d_labels);

/* Gnomix.predict_proba / predict: base + smoother with B kept on the device. */
int gnx_infer(gnx_model* model, const int8_t* X, int64_t N, int64_t ldx, float* proba_f32, double* proba_f64,
              int32_t* labels);
int gnx_infer_dev(gnx_model* model, const int8_t* dX, int64_t N, int64_t ldx, float* d_proba_f32,
                  double* d_proba_f64, int32_t* d_labels);

/* 2-bit packed haplotypes.  The reference's contract is int8 {0,1,2}, one byte per SNP (src/utils.py:153) and gnx_infer
 * keeps accepting exactly that; whole genome it is 17.7 MB per haplotype, so the 63 GB/s host link bounds the host-pointer
 * path at a few thousand haplotypes/s/GPU.  A caller that can hand over X as 2-bit fields moves a quarter of
 * the bytes: SNP j of a row lives in bits 2*(j%4)..2*(j%4)+1 of byte j/4 (value = the int8 code, 0..3), rows ldp bytes apart
 * (ldp >= ceil(C/4); gnx_packed_row_bytes(C) = the canonical stride, a multiple of 4, its tail zeroed by gnx_pack_x).
 *   gnx_pack_x          host utility: int8 (N, ldx) -> packed (N, ldp) on n_threads host threads (<= 0: all cores, at most
 *                       64); GNX_EINVAL if a value is outside 0..3.  Needs no context and no GPU.
 *   gnx_infer_packed    gnx_infer on packed host input: batches are copied, widened on the device and run through the same
 *                       kernels, H2D / kernels / D2H overlapped on three streams; results are bit-identical to gnx_infer's.
 *   gnx_unpack_x_dev    the widening pass alone, on the context stream (device pointers).
 *   gnx_infer_packed_dev  device-resident packed input.
 *   gnx_base_predict_packed_dev  Base.predict_proba (src/Base/base.py:146-180) on device-resident packed input.
 * With the logistic base (up to 32 class columns per SNP, i.e. A <= 16 at the default context) packed rows are NOT widened:
 * k_base_logistic_p2 reads the 2-bit rows and expands them to the int8 MFMA operand in registers — a quarter of the X bytes
 * through HBM and the L1s; B is bit-identical to the int8 entry points'.  Other bases widen to int8 in device scratch first. */
int64_t gnx_packed_row_bytes(int64_t C);
int gnx_pack_x(const int8_t* X, int64_t N, int64_t ldx, int64_t C, uint8_t* packed, int64_t ldp, int n_threads);
int gnx_unpack_x_dev(gnx_ctx* ctx, const uint8_t* d_packed, int64_t N, int64_t ldp, int64_t C, int8_t* dX, int64_t ldx);
int gnx_infer_packed(gnx_model* model, const uint8_t* packed, int64_t N, int64_t ldp, float* proba_f32, double* proba_f64,
                     int32_t* labels);
int gnx_base_predict_packed_dev(gnx_model* model, const uint8_t* d_packed, int64_t N, int64_t ldp, float* d_b_f32,
                                double* d_b_f64);
int gnx_infer_packed_dev(gnx_model* model, const uint8_t* d_packed, int64_t N, int64_t ldp, float* d_proba_f32,
                         double* d_proba_f64, int32_t* d_labels);

/* smoother.model.predict_proba on explicit rows (R, S*A) float32 -> (R, A) float32 (XGB only). */
int gnx_smooth_rows(gnx_model* model, const float* rows, int64_t R, float* proba);

/* Calibrator.transform on explicit rows (R, A) (float64 if proba_is_f64 else float32) -> (R, A) float64
 * (src/Smooth/Calibration.py:57-69).  GNX_ESTATE when the model carries no calibrator. */
int gnx_calibrate_rows(gnx_model* model, const void* proba, int proba_is_f64, int64_t R, double* out);

/* Gnomix.phase: for each of n_ind individuals (haplotype rows 2i, 2i+1 of X and of B) run the
 * Gnofix loop with the reference's default arguments.  X (2*n_ind, ldx) int8 is re-phased IN
 * PLACE, B (2*n_ind, W, A) float64 is read only, Y (2*n_ind, W) receives Gnofix's labels and
 * n_switches (n_ind,) (may be NULL) the number of accepted switches.
 * A calibrated model (gnx_model_set_calibrate(model, 1) with calib_* loaded) re-phases as the reference's gnofix() does with a
 * calibrated Smoother: labels are argmax(Calibrator.transform(raw)) (smoother.predict, gnofix.py:80,190), candidates are compared
 * by the RAW probabilities (smoother.model.predict_proba, gnofix.py:157).  Every gnx_gnofix* / gnx_phase_gt2* entry then runs
 * k_gnofix_opts; GNX_EUNSUPPORTED (the message names the reason) for such a model without the rank-quantised smoother copy, with
 * S < 3, or with a geometry beyond that kernel's LDS working set. */
int gnx_gnofix(gnx_model* model, int8_t* X, int64_t ldx, const double* B, int64_t n_ind, int32_t max_it,
               int32_t* Y, int32_t* n_switches);
int gnx_gnofix_dev(gnx_model* model, int8_t* dX, int64_t ldx, const double* dB, int64_t n_ind, int32_t max_it,
                   int32_t* dY, int32_t* d_n_switches);
/* the same on device-resident 2-bit rows (gnx_pack_x layout; dP 4-byte aligned, ldp a multiple of 4): the SNP blocks of the
 * windows with odd final switch parity are exchanged in the packed rows (a quarter of the bytes of the int8 matrix) */
int gnx_gnofix_packed_dev(gnx_model* model, uint8_t* d_packed, int64_t ldp, const double* dB, int64_t n_ind, int32_t max_it,
                          int32_t* dY, int32_t* d_n_switches);

/* gnofix() with the reference's search options (src/Gnofix/gnofix.py:58-208).  Options equal to the defaults (criterion
 * DISC_SMOOTH, max_center_offset 0, non_lin_s 0, prob_comp MAX, padding 1, prior_switch_prob exactly 0.5) run the same kernels as
 * gnx_gnofix and give the same bits; every other setting runs k_gnofix_opts, which reproduces the reference's behaviour:
 *   - candidates of a window w inside the centers, in np.argmax order (first maximum wins): single switches at
 *     w-max_center_offset .. w+max_center_offset, double switches [w-j, w) for j = 1 .. non_lin_s-1, [w, w+j+1) for j = 0 .. non_lin_s-1;
 *   - acceptance best * prior > orig * (1 - prior) with both products in float32 (numpy >= 2, NEP 50: the Python float is "weak");
 *   - an accepted double switch exchanges B on [j1, j2) but X only from j2 on; a single switch at window 0 exchanges B alone.
 * GNX_EINVAL (nothing written): unknown enum value, max_center_offset or non_lin_s outside [0, (S-1)/2], prior_switch_prob not
 * finite or not strictly inside (0, 1), max_it < 0, struct_bytes != sizeof(gnx_gnofix_opts).
 * GNX_EUNSUPPORTED: a smoother that is not the tree smoother (with any options, the defaults included: gnx_gnofix reports the
 * same model as GNX_ESTATE, the two entries differ in this code); non-default options with a model whose smoother has no
 * rank-quantised copy (the models the float32 Gnofix kernel serves) or whose geometry does not fit the kernel's LDS.
 * naive_switch / end_naive_switch / d of the reference are not built. */
enum { GNX_GNOFIX_CHECK_DISC_SMOOTH = 0, GNX_GNOFIX_CHECK_ALL = 1, GNX_GNOFIX_CHECK_DISC_BASE = 2, GNX_GNOFIX_CHECK_DISC_EITHER = 3 };
enum { GNX_GNOFIX_PROB_MAX = 0, GNX_GNOFIX_PROB_PROD = 1 };
typedef struct gnx_gnofix_opts {
  int32_t struct_bytes;        /* sizeof(gnx_gnofix_opts): lets the struct grow */
  int32_t max_it;
  int32_t check_criterion;     /* gnofix.py:25-45 */
  int32_t max_center_offset;   /* gnofix.py:134 */
  int32_t non_lin_s;           /* gnofix.py:135-136 */
  int32_t prob_comp;           /* gnofix.py:160-163 */
  int32_t padding;             /* gnofix.py:84: 1 = windows 1..W-1, 0 = centers only */
  int32_t reserved;
  double  prior_switch_prob;   /* gnofix.py:171 */
} gnx_gnofix_opts;
int gnx_gnofix_ex(gnx_model* model, int8_t* X, int64_t ldx, const double* B, int64_t n_ind, const gnx_gnofix_opts* opts,
                  int32_t* Y, int32_t* n_switches);
int gnx_gnofix_ex_dev(gnx_model* model, int8_t* dX, int64_t ldx, const double* dB, int64_t n_ind, const gnx_gnofix_opts* opts,
                      int32_t* dY, int32_t* d_n_switches);

/* Base.train for the logistic base (src/Base/base.py:104-127 -> per window
 * LogisticRegression(penalty="l2", C=3., solver="liblinear", max_iter=1000).fit(X_w, y_w), src/Base/models.py:12-21; called
 * twice by Gnomix.train, src/model.py:104-167): all W windows x A one-vs-rest problems (A == 2: one problem per window, as
 * sklearn) of  min_w 1/2 w'w + C_reg sum_i log(1 + exp(-y_i w'[x_i, 1]))  minimised at once on the device, float64.
 *   X (N, ldx) int8 {0,1,2}, y (N, W) int32 window labels in [0, A)  (rows = haplotypes)
 *   tol: stop a problem when |grad| <= tol * |grad at w = 0| (liblinear stops at ~1e-4 scaled by the class balance; the
 *        default 1e-9 converges to the optimum that the reference's solver approximates); max_iter bounds Newton steps and is
 *        itself clamped to 200 (a Newton-CG run takes 10-20); GNX_OK is returned even when a problem has not reached tol —
 *        check info.worst_rel_gradient
 *   coef (W, A, ldc) / intercept (W, A): HOST outputs in exactly the layout gnx_model_desc.lr_coef / lr_intercept take
 *        (A == 2: rows (-w, +w), see gnomix_amd.convert.lr_rows_from_sklearn); ldc >= M + 2 ctx + C % M
 * The unsuffixed entry point takes host X / y and stages them; _dev takes device X / y (context's device). */
typedef struct gnx_train_info {
  int32_t newton_iterations, cg_iterations, n_problems, reserved;
  double worst_rel_gradient; /* max over problems of |grad| / |grad at 0| on return */
  double objective_sum;      /* sum over problems of the objective at the returned w */
} gnx_train_info;
int gnx_train_logistic(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M,
                       int64_t ctx_snps, int32_t A, double C_reg, double tol, int32_t max_iter, double* coef, int64_t ldc,
                       double* intercept, gnx_train_info* info);
int gnx_train_logistic_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                           int64_t ctx_snps, int32_t A, double C_reg, double tol, int32_t max_iter, double* coef, int64_t ldc,
                           double* intercept, gnx_train_info* info);

/* ---- training the CovRSK SVC base (mode "best"): CovRSKBase.train (src/Base/base.py:104-127, src/Base/models.py:195-215: per
 *      window sklearn.svm.SVC(kernel=CovRSK, probability=True).fit(X_w, y_w)).  Restates sklearn's libsvm (C-SVC, C = 1, eps = 1e-3,
 *      shrinking, one model per class pair, each with Platt's 5-fold cross-validated sigmoid) on the window's exact integer Gram matrix,
 *      so the fit equals sklearn's on the same Gram and seed.
 *   X (N, ldx) int8 {0,1,2}, y (N, W) int32 labels in [0, A), W = C / M; windows of the reflect-padded rows as base.py slices them
 *     (M + 2 ctx_snps SNPs, the last one C % M more)
 *   kernel_kind: GNX_SVC_KERNEL_SUBSTRINGS = CovRSK (the CovSample(width) lengths, string_kernel.py:80-110) or
 *     GNX_SVC_KERNEL_ALL_LENGTHS = the plain string kernel (every length, string_kernel.py:5-24)
 *   seeds (W,): libsvm's random_seed of each window's fit (what sklearn drew: gnomix_amd.train.svc_seed_chain)
 *   outputs (HOST, caller-allocated), P = A (A - 1) / 2: n_sv (W); n_support (W, A); support (W, N): the first n_sv[w] entries are
 *     sklearn's support_ (rows of X, class-major); dual_coef (W, A - 1, N): the first n_sv[w] columns of each row are _dual_coef_;
 *     intercept / prob_a / prob_b (W, P) = _intercept_ / _probA / _probB
 * Refused before anything is written: a window without a row of some class (GNX_EINVAL: the reference's fit fails there), a label
 * outside [0, A) (GNX_EINVAL), GNX_SVC_KERNEL_POLY (GNX_EUNSUPPORTED: its entry is gnx_train_svc_poly), a window whose largest kernel value g(width) is not below 2^24
 * (not exact in float) or wider than 16 384 SNPs (GNX_EINVAL), N whose Gram (N^2 floats) exceeds GNX_SVC_GRAM_BUDGET (GNX_EINVAL).
 * Windows are batched so that a batch's Gram matrices stay within GNX_SVC_GRAM_BUDGET.  The _dev form takes device X / y; it reads
 * y back to the host (the problems are laid out there).  Both are synchronous. */
#define GNX_SVC_GRAM_BUDGET (8ull << 30)
typedef struct gnx_svc_train_info {
  int64_t smo_iterations;  /* over every solve: the full problems and the Platt fold problems */
  int32_t n_solves;
  int32_t n_guarded;       /* solves stopped by the hang guard (50 M iterations) or with a non-finite rho: 0 on a sound fit */
  double gram_ms, smo_ms, platt_ms;  /* device time of the passes, summed over batches */
} gnx_svc_train_info;
int gnx_train_svc(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                  int32_t A, int32_t kernel_kind, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                  double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info);
int gnx_train_svc_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t ctx_snps,
                      int32_t A, int32_t kernel_kind, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                      double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info);
/* The same with the kernel's parameters in a struct: kernel_kind as above or GNX_SVC_KERNEL_RBF (SVMBase: gamma = 0.001,
 * C = 100; the Gram is |x - y|^2 on the int8 matrix cores, Q = (float) exp(-gamma d2) from the host-built table as libsvm's
 * Qfloat, the Platt folds' held-out decision values from the double table as svm_predict_values' k_function).  C is libsvm's
 * cost (> 0, finite; the fold models get the same C, as through libsvm's weight); gamma is read for RBF only (> 0, finite,
 * GNX_EINVAL otherwise).  gnx_train_svc(..., kind, ...) == gnx_train_svc2 with {kind, 0, 1.0, 0.0}. */
typedef struct gnx_svc_params {
  int32_t kernel_kind;  /* GNX_SVC_KERNEL_* */
  int32_t reserved;
  double C;             /* 1.0 for CovRSKBase (sklearn's default), 100.0 for SVMBase */
  double gamma;         /* RBF only */
} gnx_svc_params;
int gnx_train_svc2(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                   int32_t A, const gnx_svc_params* params, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                   double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info);
int gnx_train_svc2_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t ctx_snps,
                       int32_t A, const gnx_svc_params* params, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support,
                       int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info);
/* the Platt fold permutation of an l-row class-pair problem fitted with libsvm seed `seed` (svm_binary_svc_probability: sklearn's
 * mt19937 + bounded_rand_int); host only, no context */
int gnx_svc_fold_permutation(uint32_t seed, int32_t l, int32_t* perm);
/* PolynomialStringKernelBase.train (src/Base/models.py:178-193: per window SVC(kernel=poly_kernel, probability=True).fit): arguments
 * and outputs of gnx_train_svc2 with params->kernel_kind = GNX_SVC_KERNEL_POLY (anything else: GNX_EINVAL) and params->C the cost
 * (the reference: sklearn's 1.0), plus the kernel's exponent poly_p (1.2 in the reference) and run_value, a HOST table (also for the
 * _dev form) of n_run_value >= width + 1 doubles, np.arange(n) ** p as numpy computes it (width = the last, widest window).  A pair's
 * kernel value is (long long)(np.sum(run_value[contigs]) / poly_p), contigs = the run of equal SNPs before every mismatch and the one
 * the window ends with, summed in numpy's pairwise order (k_svc_gram_poly); the solver, the Platt folds and the sigmoid fit are
 * gnx_train_svc2's.  Refused before anything is written, besides gnx_train_svc2's refusals: poly_p not finite or <= 0, run_value NULL,
 * shorter than width + 1 or with a negative or non-finite entry, a window wider than 8 191 SNPs (the run values, 8 bytes each, take
 * at most 64 KiB of LDS), kernel values (run_value[width] / poly_p) not below 2^24 (all GNX_EINVAL). */
int gnx_train_svc_poly(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                       int32_t A, const gnx_svc_params* params, double poly_p, const double* run_value, int64_t n_run_value,
                       const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support, double* dual_coef, double* intercept,
                       double* prob_a, double* prob_b, gnx_svc_train_info* info);
int gnx_train_svc_poly_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                           int64_t ctx_snps, int32_t A, const gnx_svc_params* params, double poly_p, const double* run_value,
                           int64_t n_run_value, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                           double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info);
/* The Gram matrices the string-kernel trainers solve on: gram (w1 - w0, N, N) float (HOST) = K(Xw, Xw) of windows [w0, w1), by the same
 * pack and Gram kernels.  kernel_kind GNX_SVC_KERNEL_SUBSTRINGS, GNX_SVC_KERNEL_ALL_LENGTHS (poly_p / run_value / n_run_value unread)
 * or GNX_SVC_KERNEL_POLY (as in gnx_train_svc_poly).  The trainers' bounds on the window width and the kernel values hold (GNX_EINVAL);
 * so does GNX_SVC_GRAM_BUDGET for the whole range.  Synchronous. */
int gnx_svc_gram(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx_snps, int32_t kernel_kind,
                 double poly_p, const double* run_value, int64_t n_run_value, int64_t w0, int64_t w1, float* gram);

/* ---- training the tree smoother: Smoother.train of XGB_Smoother (src/Smooth/smooth.py:28-38, src/Smooth/models.py:14-20:
 *      XGBClassifier(n_estimators=100, max_depth=4, learning_rate=0.1, reg_lambda=1, objective='multi:softprob').fit(slide_window(B), y))
 * Second-order gradient boosting of A regression trees per round on the softmax objective, in the histogram form (<= max_bin
 * quantile bins per class column; gradient sums in fixed point, so the trees do not depend on scheduling and equal the CPU
 * oracle's bit for bit).  xgboost itself is a third-party fitter outside the reference tree: this entry point reproduces the
 * algorithm the call asks for, not xgboost's floating-point trajectory.
 *   B (N, W, A) base probabilities (what Base.predict_proba returned for the smoother's training haplotypes), float32 or float64
 *   y (N, W) int32 labels in [0, A);  W >= 2 S, S odd.  gnx_train_gbt rejects labels outside the range; gnx_train_gbt_dev (arrays
 *     already in HBM) does not read them back to check: a row whose label is outside [0, A) counts as belonging to no class
 *     (labels are only ever compared, never used as an index)
 *   outputs (HOST, caller-allocated): tree_off[T+1], tree_class[T], left / right / feat (int32) and cond (float32) with room for
 *     (2^(max_depth+1) - 1) T nodes (63 T at the limit max_depth = 5), T = n_rounds * A — exactly the arrays gnx_model_desc takes (a leaf has left = right = -1 and its value in cond;
 *     tree t belongs to class t % A); *n_nodes = nodes written; loss[n_rounds + 1] (optional) = mean log loss before each round
 *     and after the last. */
typedef struct gnx_gbt_params {
  int32_t n_rounds;          /* 100  (n_estimators) */
  int32_t max_depth;         /* 4, at most 5 */
  int32_t max_bin;           /* 256, at most 256 */
  int32_t tree_method;       /* 0 = histogram (max_bin quantile bins per class column, xgboost's "hist"); 1 = exact greedy: a candidate
                                between every two distinct feature values of a node's rows (xgboost's "exact"); NaN probabilities sort as +inf */
  double eta;                /* 0.1  (learning_rate) */
  double lambda;             /* 1.0  (reg_lambda) */
  double gamma;              /* 0.0  (min_split_loss) */
  double min_child_weight;   /* 1.0 */
  double base_score;         /* 0.5 */
} gnx_gbt_params;
int gnx_train_gbt(gnx_ctx* ctx, const void* B, int32_t b_is_f64, const int32_t* y, int64_t N, int32_t W, int32_t A, int32_t S,
                  const gnx_gbt_params* params, int32_t* tree_off, int32_t* tree_class, int32_t* left, int32_t* right,
                  int32_t* feat, float* cond, int64_t* n_nodes, double* loss);
int gnx_train_gbt_dev(gnx_ctx* ctx, const void* dB, int32_t b_is_f64, const int32_t* dy, int64_t N, int32_t W, int32_t A, int32_t S,
                      const gnx_gbt_params* params, int32_t* tree_off, int32_t* tree_class, int32_t* left, int32_t* right,
                      int32_t* feat, float* cond, int64_t* n_nodes, double* loss);

/* ---- training the boosted-tree base: Base.train of XGBBase (src/Base/base.py:104-127, src/Base/models.py:24-35: per window
 *      XGBClassifier(n_estimators=20, max_depth=4, learning_rate=0.1, reg_lambda=1, reg_alpha=0, missing=2).fit(Xw, yw)).
 * Second-order boosting on the window's SNP codes, all W = C / M windows in one launch sequence per round (forest/k_train_gbt_base.hip, whose
 * header states the algorithm completely).  As for gnx_train_gbt, xgboost is a third-party fitter outside the reference tree: what is
 * reproduced is the algorithm that call asks for, NOT xgboost's floating-point trajectory (parity with xgboost itself is unpinned);
 * gradient sums are fixed point (2^-30) in int64, so the trees do not depend on scheduling and equal the CPU restatement bit for bit.
 *   X (N, ldx) int8 codes 0, 1 and 2 = missing (fb_missing), y (N, W) int32 labels in [0, A).  gnx_train_gbt_base rejects any other
 *     code and any label outside the range (GNX_EINVAL).  gnx_train_gbt_base_dev (arrays already in HBM) reads neither back: a code
 *     other than 1 or 2 trains as a 0 (codes are only compared, never used as an index) and, as in gnx_train_gbt_dev, a label outside
 *     [0, A) belongs to no class.
 *   A >= 3: multi:softprob, A trees per round, tree t of a window adds to class t % A;  A == 2: binary:logistic, one tree per round.
 *   params: n_rounds (20 for XGBBase), max_depth (4; 1..5), eta, lambda, gamma, min_child_weight, base_score (0.5).  max_bin and
 *     tree_method are ignored: a SNP has two present values, so xgboost's "hist" and "exact" enumerate the same splits.
 *   outputs (HOST, caller-allocated), the forest base's own layout, ready for gnx_model_desc (fb_*): win_tree0[W+1], tree_off[T+1],
 *     tree_class[T], left / right / feat (int32, feat = SNP index within the window's padded slice), cond (float32: 0.5 or 1.5, a
 *     leaf's value at leaves) and default_left (uint8) with room for (2^(max_depth+1) - 1) T nodes, T = W * n_rounds * (A == 2 ? 1 : A);
 *     *n_nodes = nodes written; loss[n_rounds + 1] (optional) = mean log loss over the N * W problems before each round and after
 *     the last (float64).
 * gnx_train_gbt_base_phases(enable, ms): enable = 1 / 0 makes later calls time their phases (one stream synchronisation per phase) or
 *   stops that, -1 leaves the switch; ms (5 doubles, may be NULL) receives the last timed call's milliseconds in gradients + loss,
 *   per-level sums, split search, row partition, leaves + margins.  Process-wide, for scripts/bench_train_forest.py. */
int gnx_train_gbt_base(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                       int32_t A, const gnx_gbt_params* params, int32_t* win_tree0, int32_t* tree_off, int32_t* left, int32_t* right,
                       int32_t* feat, float* cond, uint8_t* default_left, int32_t* tree_class, int64_t* n_nodes, double* loss);
int gnx_train_gbt_base_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                           int64_t ctx_snps, int32_t A, const gnx_gbt_params* params, int32_t* win_tree0, int32_t* tree_off, int32_t* left,
                           int32_t* right, int32_t* feat, float* cond, uint8_t* default_left, int32_t* tree_class, int64_t* n_nodes,
                           double* loss);
int gnx_train_gbt_base_phases(int32_t enable, double* ms);

/* ---- training the random-forest base: Base.train of RFBase (src/Base/base.py:104-127, src/Base/models.py:54-66: per window
 *      RandomForestClassifier(n_estimators=20, max_depth=4).fit(Xw, yw)), tree for tree as scikit-learn 1.7.2 builds them
 *      (forest/k_train_rforest.hip, whose header states the chain; tests/rf_exact.py restates it and is held to live scikit-learn).
 *      What numpy's generator decides is the caller's (gnomix_amd.train.rforest_bootstrap): for tree t of window w
 *        weight[w, t, n] = how often the bootstrap drew row n (uint8; GNX_EINVAL above 127: the int8 operand of the count product),
 *        state[w, t]     = the splitter's 32-bit generator state (uint32).
 *      X (N, ldx) int8 codes 0..2, y (N, W) int32 labels in [0, A), 2 <= A <= 32, N < 2^24 (GNX_EINVAL beyond: an int32 sum of
 *      weights could overflow), 1 <= max_depth <= 5.  gnx_train_rforest checks X and y (GNX_EINVAL); gnx_train_rforest_dev (X, y,
 *      weight, state already in HBM) reads neither back: codes are only compared, a label outside [0, A) belongs to no class.
 *      Outputs (HOST, caller-allocated), the rforest base's own layout, ready for gnx_model_desc (rf_*): win_tree0[W+1],
 *      tree_off[W n_trees + 1], left / right / feat (int32; children are indices inside the tree, -1 at leaves; feat = SNP index
 *      within the window's padded slice, 0 at leaves), thr (float64: 0.5, 1.0 or 1.5, -2 at leaves) with room for
 *      (2^(max_depth+1) - 1) W n_trees nodes and value with A times as many (float64, a node's class frequencies); *n_nodes = nodes
 *      written.  Trees do not depend on scheduling.
 * gnx_train_rforest_phases(enable, ms): as gnx_train_gbt_base_phases; ms (3 doubles, may be NULL) receives the last timed call's
 *   milliseconds in the count product, the draw and the row partition.  Process-wide, for scripts/bench_train_rforest.py. */
int gnx_train_rforest(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                      int32_t A, int32_t n_trees, int32_t max_depth, const uint8_t* weight, const uint32_t* state, int32_t* win_tree0,
                      int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat, double* thr, double* value, int64_t* n_nodes);
int gnx_train_rforest_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                          int64_t ctx_snps, int32_t A, int32_t n_trees, int32_t max_depth, const uint8_t* d_weight,
                          const uint32_t* d_state, int32_t* win_tree0, int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat,
                          double* thr, double* value, int64_t* n_nodes);
int gnx_train_rforest_phases(int32_t enable, double* ms);

/* ---- fitting the Naive-Bayes bases: the counting half of Base.train(X, y) for NBBernoulliBase / NBMultinomialBase /
 *      NBGaussianBase (src/Base/base.py:104-127, src/Base/models.py:96-132).  Every fitted attribute of the three estimators is a
 *      closed form of three integer tables, and the integers are exact:
 *        n1[w, c, p] = rows n with y[n, w] == c and X[n, col(w, p)] == 1        (W, A, ldw) int32, ldw = M + 2 ctx + (C - M W)
 *        n2[w, c, p] = the same for code 2                                       (W, A, ldw) int32; positions >= width_w hold 0
 *        class_count[w, c] = rows n with y[n, w] == c                            (W, A) int32
 *      (n0 = class_count - n1 - n2.)  col(w, p) is the window's slice of the reflect-padded row.  The float64 closed forms are the
 *      caller's (gnomix_amd.train.train_nb_base: scikit-learn's own expressions).
 *      X (N, ldx) int8 codes 0..2, y (N, W) labels in [0, A), 2 <= A <= 32, N < 2^31.  The host form checks X and y (GNX_EINVAL); the
 *      _dev form takes device pointers for inputs AND outputs, runs asynchronously on the context's stream, counts only codes 1 and
 *      2 and ignores rows whose label is outside [0, A). */
int gnx_train_nb_counts(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                        int32_t A, int32_t* n1, int32_t* n2, int32_t* class_count);
int gnx_train_nb_counts_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                            int64_t ctx_snps, int32_t A, int32_t* d_n1, int32_t* d_n2, int32_t* d_class_count);

/* ---- fitting the LDA base: the integer half of Base.train(X, y) for LDABase (LinearDiscriminantAnalysis(), solver "svd").
 *      Everything scikit-learn's _solve_svd consumes is a function of three exact integer quantities per window:
 *        G[w]    = Xw^T Xw                                  (ldw, ldw) int32, full symmetric, ldw = M + 2 ctx + (C - M W)
 *        S[w, k] = sum of the rows n with y[n, w] == k      (A, ldw) int32
 *        n[w, k] = number of those rows                     (A,) int32
 *      Xw = the window's slice of the reflect-padded row; positions >= width_w hold 0.  The within-class scatter is
 *      G - sum_k S_k S_k^T / n_k; the float64 rest (std, the two truncated decompositions, coef_ / intercept_) is the caller's
 *      (gnomix_amd.train.lda_finish).  One v_mfma_i32_16x16x64_i8 product of [Xw | onehot(y)] with itself gives all three.
 *      The outputs cover the windows [w0, w1) only — window w0 first — so that the caller bounds memory: (w1 - w0) ldw^2 int32.
 *      X (N, ldx) int8 codes 0..2, y (N, W) labels in [0, A), 2 <= A <= 32.  GNX_EINVAL: 4 N >= 2^31 (an int32 sum could overflow),
 *      a bad range, a NULL pointer; the host form also checks X and the range's labels (GNX_EINVAL) before anything is launched.
 *      The _dev form takes device pointers for inputs AND outputs, runs asynchronously on the context's stream, and a row whose
 *      label is outside [0, A) enters G but no class sum or count. */
int gnx_train_lda_gram(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                       int32_t A, int64_t w0, int64_t w1, int32_t* G, int32_t* S, int32_t* n);
int gnx_train_lda_gram_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                           int64_t ctx_snps, int32_t A, int64_t w0, int64_t w1, int32_t* d_G, int32_t* d_S, int32_t* d_n);

/* ---- training the convolutional smoother: CNN.fit (src/Smooth/cnn.py:104-118) as Smoother.train calls it for CNN_Smoother
 *      (src/Smooth/smooth.py:28-38, src/Smooth/models.py:35-42).  nn.Conv1d(A, A, S, padding = (S-1)/2) with zero padding,
 *      loss = NLLLoss(log(softmax + log_eps), y) averaged over the batch's rows x windows (cnn.py:57-75), torch.optim.Adam
 *      (cnn.py:32), mini-batches of `batch` rows in the order `order` gives for each epoch (the DataLoader's shuffle, cnn.py:172;
 *      NULL = 0 .. N-1 every epoch).  All arithmetic float32.
 *      B (N, W, A) float32 / float64 and y (N, W) on the host; weight (A, A, S) and bias (A) hold the initial parameters on
 *      entry (torch's default: uniform(+-1/sqrt(A*S))) and the trained ones on return; loss (epochs) receives each epoch's mean
 *      batch loss (the number cnn.py:120 prints) or may be NULL. */
typedef struct gnx_cnn_params {
  int32_t epochs;            /* 250  (max_ep) */
  int32_t batch;             /* 128  (DataLoader batch_size) */
  double lr;                 /* 1e-3 (Adam) */
  double beta1, beta2, eps;  /* 0.9, 0.999, 1e-8 (Adam defaults) */
  double log_eps;            /* 1e-8 (cnn.py:73) */
} gnx_cnn_params;
int gnx_train_cnn(gnx_ctx* ctx, const void* B, int32_t b_is_f64, const int32_t* y, int64_t N, int32_t W, int32_t A, int32_t S,
                  const gnx_cnn_params* params, const int64_t* order, float* weight, float* bias, double* loss);

/* ---- training the linear-chain CRF smoother: CRF.fit (src/Smooth/crf.py:51-58: sklearn_crfsuite.CRF(algorithm="lbfgs",
 *      max_iterations=10000, all_possible_transitions=True, all_possible_states=True)) as Smoother.train calls it for
 *      CRF_Smoother (src/Smooth/smooth.py:28-38, src/Smooth/models.py:27-32).  Minimises CRFsuite's objective
 *      f = - sum log p(y | x) + c2 |w|^2 over state (attribute, label) and transition (from, to) weights — the arrays
 *      gnx_model_desc.crf_state / crf_trans take — by L-BFGS with every evaluation on the device (k_train_crf.hip).
 *      state / trans (A, A) hold the starting point on entry (CRFsuite starts from zeros) and the fit on return. */
typedef struct gnx_crf_params {
  double c1;                 /* 0.0  (L1: only 0 is built) */
  double c2;                 /* 1.0  (L2, CRFsuite's default) */
  double epsilon;            /* 1e-8: stop when |g| / max(1, |w|) < epsilon (CRFsuite: 1e-5) */
  int32_t max_iterations;    /* 10000 (crf.py:7) */
  int32_t memory;            /* 10: L-BFGS pairs kept (CRFsuite: 6) */
} gnx_crf_params;
typedef struct gnx_crf_info {
  int32_t iterations, evaluations;
  double objective, grad_norm;
  int32_t converged, reserved;
} gnx_crf_info;
int gnx_train_crf(gnx_ctx* ctx, const void* B, int32_t b_is_f64, const int32_t* y, int64_t N, int32_t W, int32_t A,
                  const gnx_crf_params* params, double* state, double* trans, gnx_crf_info* info);

/* ---- one isotonic map of the calibrator: Calibrator.fit (src/Smooth/Calibration.py:43-55) fits, per class i,
 *      sklearn IsotonicRegression(out_of_bounds='clip') on (proba[:, i], y == class i) with float32 probabilities.
 * Host arithmetic (no context, no device): x, y (n,) float32 in any order -> thresholds x_thr / y_thr (caller-allocated, n each),
 * *n_thr of them; they go into gnx_model_desc.calib_x / calib_y (as float64) with calib_is_f32 = 1. */
int gnx_fit_isotonic_f32(const float* x, const float* y, int64_t n, float* x_thr, float* y_thr, int64_t* n_thr);
/* The same fit on float64 probabilities (the CRF smoother's; the CNN smoother's are float32 and use the entry above): ties are
 * merged below 1e-15 (numpy's float64 resolution), every sum, mean and block mean is a float64 in scikit-learn's / scipy's order of
 * operations; the thresholds go into calib_x / calib_y as they are, with calib_is_f32 = 0. */
int gnx_fit_isotonic_f64(const double* x, const double* y, int64_t n, double* x_thr, double* y_thr, int64_t* n_thr);

/* ---- the admixture simulator's training data: LAIDataset.simulate (src/laidataset.py:362-428) + admix (:119-176) write each
 *      simulated haplotype as founder slices; write_output (:180-201) stacks them; window_reshape / data_process
 *      (src/preprocess.py:37-82, called from gnomix.py:139-146) reduce the per-SNP ancestry to window labels.
 * The random draws are the host's (gnomix_amd/simulate.py); they arrive as segment tables.  Haplotype n (0 <= n < N) is the
 * segments seg_off[n] .. seg_off[n+1]-1: segment s covers SNPs seg_begin[s] .. (the next begin, or C) - 1 and copies them from
 * founder row seg_src[s] of F (n_founder_haps rows of C int8 values, ldf bytes apart; founder haplotype = 2 * sample + {0 maternal,
 * 1 paternal}).  anc_of_src[r] is row r's ancestry code; a code >= A marks a row that is not a founder (never referenced, not
 * checked).  Outputs: X (N, C) rows ldx bytes apart = mat_vcf_2d; Y (N, W) int32 window labels, W = C / M, windows 0 .. W-2 of M
 * SNPs and the last of M + C % M, label = the most frequent ancestry with ties to the smallest code (scipy.stats.mode); anc
 * (N, C) = mat_map, written only when non-NULL.
 * GNX_EINVAL, nothing written: bad sizes, 1 <= A <= GNX_SIM_MAX_A violated, seg_off[0] != 0 or a haplotype without segments, a
 * first begin != 0, begins not increasing or >= C, a source outside [0, n_founder_haps) or not a founder, a founder row holding a
 * value other than 0 / 1 (the message names the row and the SNP).  N == 0: GNX_OK, nothing launched.
 * The _dev form validates on the device and reads the verdict back (it synchronises the context stream once); the host form
 * stages everything through device memory of its own, freed before it returns. */
#define GNX_SIM_MAX_A 255
int gnx_simulate_admix_dev(gnx_ctx* ctx, const int8_t* dF, int64_t n_founder_haps, int64_t ldf, int64_t C, int64_t M,
                           const int64_t* d_seg_off, const int32_t* d_seg_begin, const int32_t* d_seg_src,
                           const uint8_t* d_anc_of_src, int32_t A, int64_t N, int8_t* dX, int64_t ldx, int32_t* dY,
                           uint8_t* d_anc);
int gnx_simulate_admix(gnx_ctx* ctx, const int8_t* F, int64_t n_founder_haps, int64_t ldf, int64_t C, int64_t M,
                       const int64_t* seg_off, const int32_t* seg_begin, const int32_t* seg_src, const uint8_t* anc_of_src,
                       int32_t A, int64_t N, int8_t* X, int64_t ldx, int32_t* Y, uint8_t* anc);

/* ---- scoring a split that was predicted on the device: the bookkeeping of Gnomix.train (src/model.py:127-151: accuracy_score,
 *      balanced_accuracy_score and confusion_matrix of sklearn on label vectors) needs only the A x A counts
 *        cm[t * A + p] = #{i : y[i] == t and pred[i] == p}
 *      (gnomix_amd/metrics.py turns them into the reference's figures).  k_confusion.hip counts them in one pass.
 *   y (n,) int32 true labels;  pred by pred_kind: (n,) int32 labels, or (n, A) float64 / float32 probabilities of which the
 *     first-maximum argmax is taken as np.argmax(B, -1) does (Base.evaluate, src/Base/base.py:221): a NaN counts as a maximum and
 *     the first NaN of a row wins;  cm (A * A) int64, overwritten.  n == 0: cm is zeroed, nothing launched.
 *   A true or predicted label outside [0, A) indexes nothing: such elements are counted apart and, after the launch, reported as
 *     GNX_EINVAL (the message gives their number); cm then holds the counts of all other elements.
 *   GNX_EUNSUPPORTED: A > GNX_CONFUSION_MAX_A (the per-workgroup table is A x A 32-bit counters in LDS).
 *   Debugging arguments (0 / NULL in production): a workgroup adds its table to cm before it has counted more than
 *     debug_flush_every elements since the last time (built in: 2^31, the bound that keeps a 32-bit counter from overflowing; at least
 *     one step of 256 elements is always counted); *debug_n_flushes receives the number of such additions over all workgroups.
 *   Both forms synchronise the context stream once (the verdict on the labels is read back). */
#define GNX_CONFUSION_MAX_A 32
enum { GNX_PRED_LABELS_I32 = 0, GNX_PRED_PROBA_F64 = 1, GNX_PRED_PROBA_F32 = 2 };
int gnx_confusion_dev(gnx_ctx* ctx, const int32_t* d_y, const void* d_pred, int pred_kind, int64_t n, int32_t A, int64_t* d_cm,
                      int64_t debug_flush_every, int64_t* debug_n_flushes);
int gnx_confusion(gnx_ctx* ctx, const int32_t* y, const void* pred, int pred_kind, int64_t n, int32_t A, int64_t* cm,
                  int64_t debug_flush_every, int64_t* debug_n_flushes);

/* ---- the window labels after the argmax (csrc/labels/k_labels.hip) ------------------------------------------------------------
 * gnx_mode_filter: Smoother.predict's mode_filter (src/Smooth/smooth.py:63-64, src/Smooth/utils.py:31-46) with the meaning it has
 *   under the scipy it was written for (< 1.11: stats.mode(arr)[0][0] is the smallest most frequent value).  in / out (N, W) int32
 *   labels in [0, A), A <= GNX_MODE_FILTER_MAX_A; the arrays must not overlap.  ends = size / 2 (an even size acts as size + 1).
 *   Position i with ends <= i < W - ends becomes the most frequent label of in[i - ends .. i + ends] when the smallest and the
 *   largest most frequent label agree, and stays in[i] otherwise; every other position (all of them for size <= 1 and for
 *   2 * ends >= W) is copied.  Windows are read from `in`, so nothing cascades.
 *   GNX_EINVAL before the launch: size < 0 (and bad sizes / pointers); GNX_EINVAL after the launch: a label outside [0, A) was met
 *   (such a label equals no class and is handed on unchanged; labels are only compared, never used as an index).
 *   A row of at most GNX_MODE_FILTER_LDS_ROW labels is staged in LDS; a longer one is read from global memory by the same kernel.
 *   Both forms synchronise the context stream once (the verdict on the labels is read back).  The _dev form takes row strides in
 *   elements (>= W). */
#define GNX_MODE_FILTER_MAX_A 32
#define GNX_MODE_FILTER_LDS_ROW 16384
int gnx_mode_filter_dev(gnx_ctx* ctx, const int32_t* d_in, int64_t ld_in, int32_t* d_out, int64_t ld_out, int64_t N, int64_t W,
                        int32_t A, int64_t size);
int gnx_mode_filter(gnx_ctx* ctx, const int32_t* in, int32_t* out, int64_t N, int64_t W, int32_t A, int64_t size);
/* gnx_label_runs: the run-length encoding get_bed_data walks out of one haplotype column (src/postprocess.py:162-193), for all
 *   rows at once.  labels (N, W) int32, rows ldl >= W elements apart (any values).  A run is a maximal stretch of equal labels of
 *   a row.  counts (N) int64 = runs per row; offsets (N + 1) int64 = their exclusive prefix, offsets[N] = *total; triples
 *   (capacity, 3) int32 = (first_window, last_window, label) of every run, row after row: row n owns triples offsets[n] ..
 *   offsets[n + 1] - 1.  Two passes (count, fill) with the prefix between them; *total (a host word) is always set.
 *   GNX_EINVAL with counts, offsets and *total written and the triples untouched: capacity < *total.  W == 0: no runs.
 *   Both forms synchronise the context stream once (the total is read back). */
int gnx_label_runs_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ldl, int64_t N, int64_t W, int64_t* d_counts, int64_t* d_offsets,
                       int32_t* d_triples, int64_t capacity, int64_t* total);
int gnx_label_runs(gnx_ctx* ctx, const int32_t* labels, int64_t ldl, int64_t N, int64_t W, int64_t* counts, int64_t* offsets,
                   int32_t* triples, int64_t capacity, int64_t* total);

/* ---- global ancestry and tract summaries of the window labels (csrc/summary/k_ancestry_summary.hip) -----------------------------
 * gnx_ancestry_summary: what an .msp is collapsed to first.  labels (N, W) int32 in [0, A), rows ld_labels >= W elements apart;
 *   proba NULL or the smoother's (N, W, A) probabilities, float32 or float64 (proba_is_f64); weights a HOST array of W float64
 *   window weights (NULL = all ones), e.g. the windows' lengths in cM.  Per row n and ancestry a, each an (N, A) array:
 *     hard          float64  (sum of w[k] over the windows with labels[n, k] == a) / (sum of all w[k])
 *     soft          float64  (sum of w[k] * proba[n, k, a]) / (sum of all w[k]); float32 values are widened before the multiply.
 *                            NULL exactly when proba is NULL
 *     tract_count   int32    number of maximal runs of label a in the row
 *     tract_total   float64  the unnormalised numerator of hard
 *     tract_longest float64  the largest sum of w over one such run (0 when there is none)
 *   Any output but soft may be NULL (not wanted).  The float64 sums are taken in one fixed order that depends on W alone (stated in
 *   the kernel file's header, restated in tests/summary_exact.py): two calls on the same input give the same bits.
 *   GNX_EINVAL before the launch, nothing written: N < 0, W < 1, A < 1, ld_labels < W, a weight that is negative or not finite,
 *     weights that sum to zero, soft and proba not both NULL or both given.
 *   GNX_EUNSUPPORTED: A > GNX_SUMMARY_MAX_A or W > GNX_SUMMARY_MAX_W (a wave stages its row in LDS, one byte per label, four rows per
 *     workgroup: 32 KB).
 *   GNX_EINVAL after the launch: a label outside [0, A) was met.  Labels are only compared, never used as an index: such a label
 *     counts for no ancestry (and ends a tract); everything else in the outputs is as stated.
 *   N == 0: nothing launched.  Both forms synchronise the context stream once (the verdict on the labels is read back). */
#define GNX_SUMMARY_MAX_A 32
#define GNX_SUMMARY_MAX_W 8192
int gnx_ancestry_summary_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, const void* d_proba, int proba_is_f64,
                             const double* weights, int64_t N, int64_t W, int32_t A, double* d_hard, double* d_soft,
                             int32_t* d_tract_count, double* d_tract_total, double* d_tract_longest);
int gnx_ancestry_summary(gnx_ctx* ctx, const int32_t* labels, int64_t ld_labels, const void* proba, int proba_is_f64,
                         const double* weights, int64_t N, int64_t W, int32_t A, double* hard, double* soft, int32_t* tract_count,
                         double* tract_total, double* tract_longest);

/* ---- ancestry-specific allele counts and per-ancestry dosage (csrc/summary/k_allele_counts.hip) ----------------------------------
 * The join of a local-ancestry call with the genotypes.  rows: X (N, C) in the model's coding, row_kind GNX_ROWS_INT8 (one byte per
 *   SNP: 0 = REF, 1 = ALT, ANY other byte, negatives included, = a missing call) or GNX_ROWS_PACKED2 (the gnx_pack_x layout: SNP j =
 *   bits 2 (j % 4).. of byte j / 4; codes 2 and 3 = missing), rows ld_rows BYTES apart (>= C, or >= ceil(C / 4) packed).  labels (N, W)
 *   int32, rows ld_labels >= W elements apart.  The window of SNP c is win(c) = min(c / M, W - 1): the last window takes the remainder
 *   C - M W.  Required: M >= 1, W >= 1, M W <= C.
 * gnx_ancestry_allele_counts: three int32 tables laid out (A, C), OVERWRITTEN (zeroed, then counted; any may be NULL):
 *     n_obs[a, c]  = #{h : labels[h, win(c)] == a and X[h, c] in {0, 1}}
 *     n_alt[a, c]  = #{h : labels[h, win(c)] == a and X[h, c] == 1}
 *     n_miss[a, c] = #{h : labels[h, win(c)] == a and X[h, c] not in {0, 1}}
 *   The frequency n_alt / n_obs is the caller's (float64, on the host).  All device arithmetic is integer: the tables are exact and do
 *   not depend on the launch geometry.  Columns past C of a packed row's last byte are not counted.
 *   debug_rows_per_chunk / debug_flush_every: 0 in production.  > 0 (tests): the rows one workgroup reduces per column tile (several
 *   workgroups then add to one tile of the tables), and the rows after which the workgroup's 8-bit counters are added to the int32
 *   tables (at most, and by default, 255).
 * gnx_ancestry_dosage: for ONE ancestry and individual i = haplotype rows 2 i, 2 i + 1, two uint8 matrices (N / 2, C), rows ld_dosage /
 *   ld_hapcount >= C bytes apart (either may be NULL):
 *     hapcount[i, c] = how many of the two haplotypes carry label `ancestry` at win(c) (0..2)
 *     dosage[i, c]   = how many of those have code 1
 *   A missing call on such a haplotype counts in hapcount and not in dosage: sum_i dosage = n_alt[ancestry], sum_i hapcount =
 *   n_obs[ancestry] + n_miss[ancestry].
 * gnx_ancestry_allele_counts_gt2: the file path's form.  G, n_variants, ldg, src as gnx_infer_gt2 takes them; the packed rows are built in
 *   HBM batch by batch as there (column map, REF flip, missing rule) and counted against the HOST labels (N, W) (contiguous rows) with
 *   the model's C, M, W and A; the (N, C) matrix never exists on the host.  A model SNP the query lacks is missing in every row.
 * GNX_EINVAL before the launch, nothing written: N < 0 or N >= 2^31, C < 1, A < 1, M < 1, W < 1, M W > C, a row stride too small, an
 *   unknown row_kind, a negative debug argument; for the dosage also odd N and ancestry outside [0, A).
 * GNX_EUNSUPPORTED: A > GNX_ALLELE_MAX_A (labels are staged as bytes and one workgroup holds 3 A KiB of counters), A C >= 2^31.  There
 *   is no limit on M or W: a tile of 1024 columns that spans many windows (small M) only stages fewer rows per batch.
 * GNX_EINVAL after the launch: labels outside [0, A) were met (the message says how many).  Labels are only compared, never used as an
 *   index: such a label counts for no ancestry; everything else in the outputs is as stated.
 * N == 0: the tables are zeroed, nothing is launched.  Every form synchronises the context stream once (the verdict on the labels). */
enum { GNX_ROWS_INT8 = 0, GNX_ROWS_PACKED2 = 1 };
#define GNX_ALLELE_MAX_A 32
int gnx_ancestry_allele_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels,
                                   int64_t ld_labels, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t* d_n_obs,
                                   int32_t* d_n_alt, int32_t* d_n_miss, int64_t debug_rows_per_chunk, int64_t debug_flush_every);
int gnx_ancestry_allele_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels,
                               int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t* n_obs, int32_t* n_alt, int32_t* n_miss,
                               int64_t debug_rows_per_chunk, int64_t debug_flush_every);
int gnx_ancestry_dosage_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                            int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, uint8_t* d_dosage, int64_t ld_dosage,
                            uint8_t* d_hapcount, int64_t ld_hapcount);
int gnx_ancestry_dosage(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                        int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, uint8_t* dosage, int64_t ld_dosage, uint8_t* hapcount,
                        int64_t ld_hapcount);
int gnx_ancestry_allele_counts_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                                   const int32_t* labels, int32_t* n_obs, int32_t* n_alt, int32_t* n_miss);

/* ---- ancestry-specific association: the sufficient statistics of the Tractor model (csrc/summary/k_ancestry_assoc.hip) -------------
 * THE MODEL.  rows, labels, M, W, A, win(c) as above; gnx_ancestry_assoc_stats takes int8 rows X only, the _dev form either row_kind.
 *   Per individual i (haplotype rows 2 i, 2 i + 1): a phenotype y[i] (float64), covariates Z[i, :K] (float64, row-major, contiguous; the
 *   CALLER supplies the intercept column; 1 <= K <= GNX_ASSOC_MAX_K) and a byte use[i] (0 = takes no part; use == NULL = all ones).
 *   Per SNP c and ancestry a, h[i, a] and d[i, a] are EXACTLY gnx_ancestry_dosage's hapcount and dosage of that ancestry: a missing
 *   call carries its label in h and adds nothing to d.
 *   Individual i takes part at window k when use[i] != 0, y[i] and Z[i, :] are finite and both its labels at k lie in [0, A).
 *   At SNP c, over the n individuals that take part at win(c):   y = Z g + sum_{a < A-1} alpha_a h_a + sum_a beta_a d_a + e   (OLS).
 *   Column rule (integers only, hence exact): a hapcount column with sum_i h[i, a] == 0 is dropped; a dosage column with
 *   sum_i d[i, a] < min_ac is dropped (min_ac >= 1) and its term reports NaN.  If the normal matrix of the kept columns is not positive
 *   definite in the host's Cholesky (gnomix_amd/assoc.py: a pivot of the unit-diagonal matrix <= 2^-40) the SNP has status 1 and NaN
 *   results; with df = n - p_kept < 1 it has status 2 and NaN results; else status 0.  Per (c, a): beta, se = sqrt(s2 (X^T X)^-1_jj)
 *   with s2 = RSS / df, t = beta / se, n_alt = sum d, n_hap = sum h (int32).  Per c: n, df, n_miss, status.
 * THE STATISTICS these entries write, for the SNPs [c0, c1) and the windows w0 = win(c0) .. w1 = win(c1 - 1), all OVERWRITTEN, one
 *   owner per value, plain stores; the finish is the host's (gnomix_amd/assoc.py).  With K1 = K + 1 and P1 = K + A:
 *     snp_f64 (c1 - c0, A, K1)   [a, k < K] = sum_i d[i, a] Z[i, k]  (D^T Z),   [a, K] = sum_i d[i, a] y[i]  (D^T y)
 *     snp_i32 (c1 - c0, NI), NI = A (A + 1) / 2 + A (A - 1) + A + 1:   D^T D (upper triangle, row-major: (0,0) .. (0,A-1), (1,1) ..),
 *                                then D^T H ([a][b < A - 1] = sum_i d[i, a] h[i, b]), then sum_i d[i, a] [A], then n_miss: the missing
 *                                calls at c on the haplotypes of the individuals that take part
 *     win_f64 (w1 - w0 + 1, P1, P1)   the Gram matrix of U = [Z, h_0 .. h_{A-2}, y]: R^T R, R^T y and y^T y for R = [Z, h_0 .. h_{A-2}]
 *     win_i32 (w1 - w0 + 1, 1 + A)    n, then sum_i h[i, a] for EVERY a < A
 *   The integers are exact.  Every float64 sum runs over the individuals in ascending i, one product per individual rounded once, no
 *   fused multiply-add: the values are a function of the inputs alone, not of the grid, of [c0, c1) or of the row form.
 * GNX_EINVAL before the launch, nothing written: odd N, N < 0, K < 1, min_ac < 1 (min_ac is only validated here: the column rule is
 *   the finish's), M < 1, W < 1, M W > C, not 0 <= c0 < c1 <= C, a stride too small, an unknown row_kind, a null pointer (use and
 *   n_bad may be NULL).  GNX_EUNSUPPORTED: A > GNX_ALLELE_MAX_A, K > GNX_ASSOC_MAX_K, N > 2^28 (the integer blocks are int32).
 * GNX_EINVAL after the launch: labels outside [0, A) were met among ALL rows at the windows w0 .. w1; *n_bad is their count (0
 *   otherwise).  Labels are only compared: such an individual takes no part at that window and every value is as stated.
 * Both forms synchronise the context stream once.  In the _dev form every pointer but n_bad is a device pointer.
 * gnx_ancestry_assoc_stats_gt2: the file path's form.  G, n_variants, ldg, src as gnx_infer_gt2 takes them; the packed rows are built in
 *   HBM batch by batch as there and reduced against the HOST labels (N, W) (contiguous rows), y, Z, use with the model's C, M, W and A;
 *   a batch holds whole individuals in ascending order and goes on from the blocks of the batches before it, so every running sum is
 *   the one a single launch makes: the blocks equal gnx_ancestry_assoc_stats' of the vcf_to_npy matrix bit for bit, whatever the batch
 *   size.  A model SNP the query lacks is missing in every row.  Also GNX_EINVAL before the launch: a column map entry outside G.
 * NOTE on status 1.  The hapcount columns h_0 .. h_{A-2} of the individuals that take part sum to 2 - h_{A-1}.  In a window where NO
 *   participant carries ancestry A - 1 they sum to twice the intercept column, the kept design is rank-deficient and EVERY SNP of that
 *   window has status 1 (the column rule only drops hapcount columns that are zero, and A - 1 has none to drop).  With many ancestries
 *   and few individuals this is common; order the populations so that the last one is present everywhere, or expect those windows. */
#define GNX_ASSOC_MAX_K 16
int gnx_ancestry_assoc_stats_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                 int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_y, const double* d_Z, int32_t K,
                                 const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1, double* d_snp_f64, int32_t* d_snp_i32,
                                 double* d_win_f64, int32_t* d_win_i32, int64_t* n_bad);
int gnx_ancestry_assoc_stats(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                             int64_t M, int64_t W, int32_t A, const double* y, const double* Z, int32_t K, const uint8_t* use,
                             int32_t min_ac, int64_t c0, int64_t c1, double* snp_f64, int32_t* snp_i32, double* win_f64, int32_t* win_i32,
                             int64_t* n_bad);
int gnx_ancestry_assoc_stats_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                                 const int32_t* labels, const double* y, const double* Z, int32_t K, const uint8_t* use, int32_t min_ac,
                                 int64_t c0, int64_t c1, double* snp_f64, int32_t* snp_i32, double* win_f64, int32_t* win_i32,
                                 int64_t* n_bad);

/* ---- ancestry-specific association for MANY quantitative traits at once: the trait-dependent statistics on the float64 matrix cores --
 * (csrc/summary/k_ancestry_assoc_traits.hip)
 * Everything not stated here is EXACTLY as gnx_ancestry_assoc_stats has it: rows, labels, M, W, A, win(c), h[i, a], d[i, a], Z, K, use,
 *   min_ac, [c0, c1), the row forms, the model, the column rule, status 1 and 2, n, df, n_alt, n_hap and n_miss.
 * INPUTS.  Y (N / 2, T) float64, row-major with row stride ldy >= T (in elements), 1 <= T <= GNX_ASSOC_MAX_T: column t is trait t.
 * PARTICIPATION.  Individual i takes part at window k when use[i] != 0, Z[i, :] is finite, EVERY entry of Y[i, :] is finite and both its
 *   labels at k lie in [0, A): complete cases across the batch of traits (for T = 1 exactly gnx_ancestry_assoc_stats' rule).  A trait's
 *   own missingness pattern is not modelled: the caller groups traits by pattern and calls once per group.
 * THE MODEL, per SNP c and trait t: gnx_ancestry_assoc_stats' model with y = Y[:, t] over the participants.  The integer quantities, the
 *   column rule and the status do not depend on t; neither do D^T Z, D^T D, D^T H and the Gram matrix of [Z, h_0 .. h_{A-2}].  These
 *   entries do NOT write them: gnx_ancestry_assoc_stats with use'[i] = use[i] && (Y[i, :] all finite) and a zero phenotype gives exactly
 *   those blocks under exactly this participation (gnomix_amd/assoc.py: finish_traits factors once per SNP and solves all T traits).
 * THE STATISTICS these entries write, for the SNPs [c0, c1) and the windows w0 = win(c0) .. w1 = win(c1 - 1), all OVERWRITTEN, one owner
 *   per value, plain stores.  With ldt = T rounded up to a multiple of 16 and P = K + A - 1, sums over the participants of the window:
 *     snp_y  (c1 - c0, A, ldt)      [a, t] = sum_i d[i, a] Y[i, t]                                  (D^T Y)
 *     win_y  (w1 - w0 + 1, P, ldt)  [p, t] = sum_i u[i, p] Y[i, t],  u = [Z, h_0 .. h_{A-2}]         ([Z, H]^T Y)
 *     win_yy (w1 - w0 + 1, ldt)     [t]    = sum_i Y[i, t]^2                                       (diag(Y^T Y))
 *   Columns t >= T of every block are written as 0.0.  No NaN or infinity enters a sum: an entry all of whose terms are zero is 0.0.
 * SUMMATION ORDER.  d * Y with d in {0, 1, 2} is exact.  snp_y: v_mfma_f64_16x16x4_f64 over the individuals in ascending groups of 4
 *   (i = 4 g .. 4 g + 3; individuals that take no part enter as zeros), the accumulator starting at +0.0; the order of the four terms
 *   inside one instruction is the hardware's and is not documented, so snp_y is NOT promised to equal gnx_ancestry_assoc_stats' D^T y bit
 *   for bit (DESIGN.md 4.23 records what was observed).  win_y and win_yy: ascending i, one product per participant rounded once, no
 *   fused multiply-add.  Every value is a function of N and the data alone: not of the grid, the tile sizes, [c0, c1) or the row form
 *   (a sub-range equals the slice of the whole range, int8 rows equal 2-bit rows, bit for bit).
 * GNX_ASSOC_MAX_T = 65536: the kernels index a window's (P + 1) ldt entries with an int (48 * 2^16 < 2^31) and put (ancestry groups) x
 *   (groups of 4 trait tiles) <= 4 * 1024 on grid.y (< 65536).  The blocks of one call are the caller's to size: chunk the SNPs.
 * GNX_EINVAL before the launch, nothing written: as gnx_ancestry_assoc_stats, and T < 1 or ldy < T.  GNX_EUNSUPPORTED:
 *   A > GNX_ALLELE_MAX_A, K > GNX_ASSOC_MAX_K, T > GNX_ASSOC_MAX_T, N > 2^28.
 * GNX_EINVAL after the launch: labels outside [0, A) among ALL rows at the windows w0 .. w1, *n_bad their count; labels are only
 *   compared, such an individual takes no part at that window and every value is as stated.
 * Both forms synchronise the context stream once.  In the _dev form every pointer but n_bad is a device pointer.
 * gnx_ancestry_assoc_traits_gt2: the file path's form, arguments as gnx_ancestry_assoc_stats_gt2.  The packed rows are built batch by
 *   batch; a batch holds whole groups of 4 individuals (8 haplotypes) whatever GNX_HOST_BATCH says and goes on from the accumulators
 *   of the batches before it, so the blocks equal gnx_ancestry_assoc_traits' of the vcf_to_npy matrix bit for bit at any batch size. */
#define GNX_ASSOC_MAX_T 65536
int gnx_ancestry_assoc_traits_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                  int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_Y, int64_t ldy, int32_t T,
                                  const double* d_Z, int32_t K, const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1, double* d_snp_y,
                                  double* d_win_y, double* d_win_yy, int64_t* n_bad);
int gnx_ancestry_assoc_traits(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                              int64_t M, int64_t W, int32_t A, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K,
                              const uint8_t* use, int32_t min_ac, int64_t c0, int64_t c1, double* snp_y, double* win_y, double* win_yy,
                              int64_t* n_bad);
int gnx_ancestry_assoc_traits_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                                  const int32_t* labels, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K,
                                  const uint8_t* use, int32_t min_ac, int64_t c0, int64_t c1, double* snp_y, double* win_y, double* win_yy,
                                  int64_t* n_bad);

/* ---- admixture mapping: the statistics of the regression of T traits on the LOCAL ANCESTRY itself, from the labels alone ------------
 * (csrc/summary/k_ancestry_assoc_admix.hip; the finish and the max-T permutations: gnomix_amd/admixmap.py)
 * An addition: nothing that existed changes, so GNX_ABI_VERSION stays 16 (as for gnx_fit_isotonic_f64).
 * INPUTS.  labels (N, W) int32 with row stride ld_labels >= W, rows 2 i and 2 i + 1 are individual i; Y (N / 2, T) float64 with row stride
 *   ldy >= T, 1 <= T <= GNX_ASSOC_MAX_T; Z (N / 2, K) float64, contiguous, the CALLER supplies the intercept column, 1 <= K <=
 *   GNX_ASSOC_MAX_K; use (N / 2,) bytes or NULL (all ones).  There are no genotypes.
 * PARTICIPATION.  Individual i takes part at window k when use[i] != 0, Z[i, :] is finite, EVERY entry of Y[i, :] is finite and both its
 *   labels at k lie in [0, A) (gnx_ancestry_assoc_traits' rule with the genotypes taken out).  h_a[i, k] in {0, 1, 2}: how many of i's two
 *   haplotypes carry label a at window k.
 * THE STATISTICS, for the windows [w0, w1), nw = w1 - w0, all OVERWRITTEN, one owner per value, plain stores; sums over the participants
 *   of the window; ldt = T rounded up to a multiple of 16:
 *     win_i  (nw, 1 + A + A (A + 1) / 2) int32      n, then hs[a] = sum_i h_a, then sum_i h_a h_b for a <= b (row by row)
 *     win_g  (nw, K (K + 1) / 2 + K A) float64      the upper triangle of Z^T Z row by row, then Z^T H ([k][a])
 *     win_y  (nw, K + A, ldt) float64               [Z, h_0 .. h_{A-1}]^T Y (ALL A ancestry columns: the host forms any sub-model)
 *     win_yy (nw, ldt) float64                      diag(Y^T Y)
 *   Columns t >= T are written as 0.0.  The integers are exact.  No NaN or infinity enters a sum: an entry all of whose terms are zero
 *   is 0.0.
 * SUMMATION ORDER.  Every float64 sum starts at +0.0 and runs over the individuals in ascending groups of 4 (i = 4 g .. 4 g + 3), one
 *   v_mfma_f64_16x16x4_f64 per group; individuals that take no part enter as zeros; the order of the four terms inside one instruction
 *   is the hardware's.  A value is a function of N and the data alone: not of the grid, the tile sizes, [w0, w1), ld_labels or ldy (a
 *   sub-range of windows equals the slice of the whole range and the host form equals the _dev form, bit for bit).
 * GNX_EINVAL before the launch, nothing written: N < 0, W < 1, A < 1, K < 1, T < 1, a stride too small, not 0 <= w0 < w1 <= W, a null
 *   pointer (use and n_bad may be NULL).  GNX_EUNSUPPORTED, nothing written: A > GNX_ALLELE_MAX_A, K > GNX_ASSOC_MAX_K,
 *   T > GNX_ASSOC_MAX_T, N > 2^28, N odd.
 * GNX_EINVAL after the launch: labels outside [0, A) among ALL rows at the windows [w0, w1), *n_bad their count (0 otherwise); labels are
 *   only compared, such an individual takes no part at that window and every value is written as stated.
 * Both forms synchronise the context stream once.  In the _dev form every pointer but n_bad is a device pointer. */
int gnx_ancestry_admixmap_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, int64_t N, int64_t W, int32_t A, const double* d_Y,
                              int64_t ldy, int32_t T, const double* d_Z, int32_t K, const uint8_t* d_use, int64_t w0, int64_t w1, int32_t* d_win_i,
                              double* d_win_g, double* d_win_y, double* d_win_yy, int64_t* n_bad);
int gnx_ancestry_admixmap(gnx_ctx* ctx, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t W, int32_t A, const double* Y, int64_t ldy,
                          int32_t T, const double* Z, int32_t K, const uint8_t* use, int64_t w0, int64_t w1, int32_t* win_i, double* win_g,
                          double* win_y, double* win_yy, int64_t* n_bad);

/* ---- ancestry-specific association for case / control traits: one logistic fit per SNP, on the device ---------------------------------
 * (csrc/summary/k_ancestry_assoc_logit.hip)
 * Everything not stated here is EXACTLY as gnx_ancestry_assoc_stats has it: rows, labels, M, W, A, win(c), h[i, a], d[i, a], y, Z, K, use,
 *   the handling of missing calls and of labels outside [0, A).
 * PARTICIPATION.  Individual i takes part at window k as above.  A participant's y[i] must be exactly 0.0 (control) or 1.0 (case): if any
 *   individual with use[i] != 0 and a finite y[i] has another value, the entry returns GNX_EINVAL BEFORE any fit, *n_bad is the count of
 *   such individuals, the message says so and the outputs are untouched.
 * THE MODEL.  At SNP c, over the n participants of win(c), by maximum likelihood:
 *     logit P(y = 1) = Z g + sum_{a < A-1} alpha_a h_a + sum_a beta_a d_a
 *   theta = (g [K], alpha [A - 1], beta [A]): Q = K + 2 A - 1 columns X; the first P = K + A - 1 are U = [Z, h_0 .. h_{A-2}].
 * COLUMN RULE (integers only, hence exact).  A hapcount column with sum_i h[i, a] == 0 is dropped.  A dosage column is kept iff
 *   sum_i d[i, a] >= min_ac AND 0 < sum_i d[i, a] y[i] < sum_i d[i, a] (at least one ALT copy among the cases and one among the
 *   controls: a one-sided allele would separate the data and take the SNP's other ancestries with it); a dropped dosage term reports
 *   NaN.  A dropped column's theta stays 0.
 * THE WINDOW'S NULL MODEL.  U alone (kept columns) is fitted once per window from theta = 0; the SNP's fit starts from the null theta
 *   with beta = 0.
 * EVALUATION at a theta, per participant, in float64 without fused multiply-add: eta = sum_j x_j theta_j (ascending j, zero x_j
 *   skipped); e = exp(-|eta|) (csrc/gnx_exp.h); q = 1 / (1 + e); mu = q or e q and 1 - mu = e q or q (eta >= 0 or < 0); w = (e q) q;
 *   the deviance term is 2 (max(t, 0) + log1p(e)) with t = -eta for a case, eta for a control.  dev = sum of the terms (-2 loglik),
 *   g = X^T (y - mu), H = X^T W X: every sum over the participants in ascending i, one term per individual ((w x_j) x_k for H, j >= k),
 *   rounded once, added to the running sum.  The order depends on N alone.
 * ITERATION (fixed, so that results are reproducible), at most max_iter steps:
 *   1. g and H at the current theta.  2. H to unit diagonal (s_j = sqrt(H_jj); a dropped column is a unit row), Cholesky; a pivot
 *   <= 2^-40 or not finite, or a kept column with H_jj <= 0: status 1.  3. delta = H^-1 g, lambda2 = g^T delta.  4. lambda2 <= tol: take
 *   the full step and stop; H is evaluated once more at the returned theta for the standard errors, dev is the deviance there (no
 *   deviance comparison on this step).  5. Otherwise the trial theta + t delta, t = 1, is halved at most 10 times while its deviance
 *   is not below the current one, then taken.  iters counts the steps taken (the last one included).
 * STATUS per SNP: 0 fitted; 1 Hessian not positive definite; 2 df = n - p_kept < 1; 3 no finite optimum (max_iter steps without
 *   lambda2 <= tol, or some participant has w_i < 2^-40 at the returned theta: fitted probabilities numerically 0 or 1, separation);
 *   4 the window's null model has status0 != 0 (status0 is 0, 1, 2 or 3 by the same rules; e.g. all participants are cases).  Status 4 is
 *   tested before 2.  beta, se, dev and theta are NaN whenever status != 0; theta0 and dev0 whenever status0 != 0.  The NOTE on status 1
 *   above applies: a window where no participant carries ancestry A - 1 has status0 1, its SNPs status 4.
 * OUTPUTS for the SNPs [c0, c1) and the windows win(c0) .. win(c1 - 1), all OVERWRITTEN, one owner per value, plain stores:
 *     snp_f64 (c1 - c0, 2 A + 1)   beta [A], se [A] (se_j = sqrt((X^T W X)^-1_jj)), dev
 *     snp_i32 (c1 - c0, 2 A + 3)   n_alt [A] = sum_i d[i, a], n_alt_case [A] = sum_i d[i, a] y[i], n_miss, iters, status
 *     theta   (c1 - c0, Q)         optional (NULL: not written): the fitted theta, 0 at a dropped column
 *     win_f64 (nw, P + 1)          theta0 [P], dev0
 *     win_i32 (nw, A + 4)          n, n_case, sum_h [A], iters0, status0
 *   n_alt, n_miss, n and sum_h equal gnx_ancestry_assoc_stats' integers on the same inputs.  A SNP's results are a function of its
 *   column, its window's labels, y, Z, use, N, A, K, min_ac, tol and max_iter alone: not of [c0, c1), the grid or the row form.
 * GNX_EINVAL before the launch, nothing written: as gnx_ancestry_assoc_stats, and tol not finite or < 0, max_iter < 1 (callers use
 *   GNX_ASSOC_LOGIT_TOL and GNX_ASSOC_LOGIT_MAX_ITER).  GNX_EUNSUPPORTED, nothing written: K > GNX_ASSOC_MAX_K or
 *   Q > GNX_ASSOC_LOGIT_MAX_Q (the message names both numbers; A <= 16 with K <= 16 runs), N > 2^28.
 * GNX_EINVAL after the launch: labels outside [0, A) among all rows at the range's windows; *n_bad is their count; every value is as
 *   stated (such an individual takes no part at that window).
 * gnx_ancestry_assoc_logit_gt2: the file path's form, arguments as gnx_ancestry_assoc_stats_gt2.  A Newton step needs every individual,
 *   so the packed rows of ALL individuals are built in HBM (N ceil(C / 4) bytes, 64-byte aligned rows); GNX_HOST_BATCH only governs how
 *   they are built: the results equal gnx_ancestry_assoc_logit's of the vcf_to_npy matrix bit for bit.
 * OUT OF SCOPE: Firth or otherwise penalised fits, score tests, mixed models and relatedness, several devices. */
#define GNX_ASSOC_LOGIT_MAX_Q 47
#define GNX_ASSOC_LOGIT_TOL 1e-10
#define GNX_ASSOC_LOGIT_MAX_ITER 25
int gnx_ancestry_assoc_logit_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                 int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_y, const double* d_Z, int32_t K,
                                 const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1, double tol, int32_t max_iter, double* d_snp_f64,
                                 int32_t* d_snp_i32, double* d_theta, double* d_win_f64, int32_t* d_win_i32, int64_t* n_bad);
int gnx_ancestry_assoc_logit(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                             int64_t M, int64_t W, int32_t A, const double* y, const double* Z, int32_t K, const uint8_t* use,
                             int32_t min_ac, int64_t c0, int64_t c1, double tol, int32_t max_iter, double* snp_f64, int32_t* snp_i32,
                             double* theta, double* win_f64, int32_t* win_i32, int64_t* n_bad);
int gnx_ancestry_assoc_logit_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                                 const int32_t* labels, const double* y, const double* Z, int32_t K, const uint8_t* use, int32_t min_ac,
                                 int64_t c0, int64_t c1, double tol, int32_t max_iter, double* snp_f64, int32_t* snp_i32, double* theta,
                                 double* win_f64, int32_t* win_i32, int64_t* n_bad);

/* ---- ancestry-partitioned polygenic scores ("partial PRS"), fused on the device (csrc/summary/k_ancestry_score.hip) -----
 * INPUTS.  rows, row_kind (GNX_ROWS_INT8 / GNX_ROWS_PACKED2), the codes (0 = REF, 1 = ALT, anything else = a missing call), labels (N, W)
 *   int32, ld_rows, ld_labels, win(c) = min(c / M, W - 1) and the requirement M W <= C are EXACTLY gnx_ancestry_allele_counts'.  Also:
 *     weights (C, A, S) float64, C-contiguous, 1 <= S <= GNX_SCORE_MAX_S (a caller with more scores calls in chunks of S);
 *     effect (C,) uint8: 1 = the effect allele of SNP c is ALT (code 1), 0 = it is REF (code 0), 255 = the SNP is not scored.
 * OUTPUTS.  Individual i is haplotype rows 2 i, 2 i + 1.  Every output is OVERWRITTEN (one owner per value, plain stores) and any may be
 *   NULL.  With "h of i" = h in {2 i, 2 i + 1}:
 *     score    (N / 2, A, S) float64   sum of weights[c, a, s] over the SNPs c with effect[c] != 255 and the h of i with
 *                                      labels[h, win(c)] == a and X[h, c] == effect[c]
 *     n_effect (N / 2, A) int32        the number of such (h, c) pairs
 *     n_scored (N / 2, A) int32        the pairs with labels[h, win(c)] == a, effect[c] != 255 and X[h, c] in {0, 1}: the denominator
 *                                      of an averaged score
 *     n_miss   (N / 2, A) int32        the pairs with labels[h, win(c)] == a, effect[c] != 255 and a missing call
 * SUMMATION ORDER.  The integers are exact.  The float64 sums are taken in ONE order, a function of (C, M, W) alone, in two levels:
 *     1. per haplotype h and window k with a = labels[h, k] in [0, A): a partial p[h, k, s] starts at +0.0 and adds weights[c, a, s] over
 *        the SNPs c of window k with effect[c] != 255 and X[h, c] == effect[c], in ASCENDING c;
 *     2. per (i, a, s): the score starts at +0.0 and adds, in ASCENDING k, first p[2 i, k, s] if labels[2 i, k] == a, then
 *        p[2 i + 1, k, s] if labels[2 i + 1, k] == a.
 *   One rounding per add, no fused multiply-add, terms that do not apply are skipped.  The order, and so every bit of score, does not
 *   depend on N (an individual's values are those of a call with that individual alone), on the grid or the tile sizes, on the row
 *   form, on the file path's batches or on the debug arguments.
 *   debug_windows_per_block / debug_rows_per_pass: 0 in production.  > 0 (tests): the windows one workgroup walks, and the rows whose
 *   partials share the workspace at a time (rounded down to a multiple of 256, at least 256).
 * GNX_EINVAL before the launch, nothing written: the conditions of gnx_ancestry_allele_counts (N < 0 or >= 2^31, C < 1, A < 1, M < 1,
 *   W < 1, M W > C, a stride too small, an unknown row_kind, a negative debug argument), odd N, S < 1, a null weights or effect; an
 *   effect byte outside {0, 1, 255}; a weight that is not finite at a SNP with effect[c] != 255 (a small checking pass over the device
 *   copies counts both and the count is read back: the message names it).
 * GNX_EUNSUPPORTED, nothing written: A > GNX_ALLELE_MAX_A, S > GNX_SCORE_MAX_S, C >= 2^30 (the counts are int32).
 * GNX_EINVAL after the launch, *n_bad set (0 otherwise; n_bad may be NULL): labels outside [0, A) were met, *n_bad of them.  Labels are only
 *   compared, never used as an index: such a haplotype counts for no ancestry at that window; every output is as stated.
 * N == 0: nothing is launched, nothing is written.  Every form synchronises the context stream twice (the checking pass, the labels).
 * In the _dev form every pointer but n_bad is a device pointer.
 * gnx_ancestry_score_gt2: the file path's form.  G, n_variants, ldg, src as gnx_infer_gt2 takes them; the packed rows are built in HBM
 *   batch by batch as gnx_ancestry_allele_counts_gt2 builds them and scored against the HOST labels (N, W) (contiguous rows) with the
 *   model's C, M, W and A.  A batch holds whole individuals, so the outputs equal the matrix path's bit for bit whatever GNX_HOST_BATCH
 *   is.  A model SNP the query lacks is missing in every row.  Also GNX_EINVAL before the launch: a column map entry outside G. */
#define GNX_SCORE_MAX_S 16
int gnx_ancestry_score_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                           int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_weights, int32_t S, const uint8_t* d_effect,
                           double* d_score, int32_t* d_n_effect, int32_t* d_n_scored, int32_t* d_n_miss, int64_t debug_windows_per_block,
                           int64_t debug_rows_per_pass, int64_t* n_bad);
int gnx_ancestry_score(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                       int64_t C, int64_t M, int64_t W, int32_t A, const double* weights, int32_t S, const uint8_t* effect, double* score,
                       int32_t* n_effect, int32_t* n_scored, int32_t* n_miss, int64_t debug_windows_per_block, int64_t debug_rows_per_pass,
                       int64_t* n_bad);
int gnx_ancestry_score_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                           const int32_t* labels, const double* weights, int32_t S, const uint8_t* effect, double* score, int32_t* n_effect,
                           int32_t* n_scored, int32_t* n_miss, int64_t* n_bad);

/* ---- ancestry-specific pairwise counts on the int8 matrix cores (csrc/summary/k_ancestry_pairs.hip) ----------------------
 * INPUTS.  rows, row_kind, the codes, labels (N, W) int32, ld_rows, ld_labels, M, W, A, win(c) = min(c / M, W - 1) and the requirement
 *   M W <= C are EXACTLY gnx_ancestry_allele_counts'.  The n = N / 2 individuals are the haplotype rows 2 i, 2 i + 1.  For ONE ancestry
 *   `ancestry`, individual i and SNP c:
 *     o[i, c] = how many of the two haplotypes h have labels[h, win(c)] == ancestry AND an observed call (code 0 or 1)      0..2
 *               (NOT gnx_ancestry_dosage's hapcount, which also counts the missing calls)
 *     d[i, c] = how many of those haplotypes have code 1                                                                   0..o[i, c]
 * OUTPUTS.  Over the SNP range [c0, c1) three (n, n) int32 tables, rows ld >= n ELEMENTS apart, OVERWRITTEN (the n columns of the n rows;
 *   what lies between n and ld is not touched); any may be NULL:
 *     DD[i, j] = sum_c d[i, c] d[j, c]   (symmetric)
 *     DO[i, j] = sum_c d[i, c] o[j, c]   (NOT symmetric)
 *     OO[i, j] = sum_c o[i, c] o[j, c]   (symmetric)
 *   Every term lies in 0..4, so int32 is exact while 4 (c1 - c0) < 2^31.  All device arithmetic is integer: the tables do not depend on
 *   the grid, the tile sizes, the row form or the debug argument, and the tables of a partition of a range add up to the range's.
 *   For i != j the caller derives mism[i, j] = DO[i, j] + DO[j, i] - 2 DD[i, j], the mismatching pairs of ancestry-labelled haplotypes one
 *   from i and one from j, comp[i, j] = OO[i, j], the pairs compared, and the allele-sharing distance mism / comp (gnomix_amd/asmds.py).
 *   debug_snps_per_block: 0 in production (the split of the SNP range over workgroups is taken from n and c1 - c0).  > 0 (tests): the
 *   SNPs one workgroup walks, rounded up to the kernel's chunk of 128.
 * GNX_EINVAL before any launch, nothing written: the conditions of gnx_ancestry_allele_counts (N < 0 or >= 2^31, C < 1, A < 1, M < 1,
 *   W < 1, M W > C, a stride too small, an unknown row_kind), odd N, ancestry outside [0, A), c0 < 0, c1 <= c0, c1 > C, ld < N / 2, a
 *   negative debug argument.
 * GNX_EUNSUPPORTED, nothing written: A > GNX_ALLELE_MAX_A, c1 - c0 >= 2^29, more than 2^31 - 1 workgroups (tile pairs x SNP segments).
 *   The index arithmetic is 64-bit throughout: there is no limit on N / 2 other than the tables' size.
 * GNX_EINVAL after the launch, *n_bad set (0 otherwise; n_bad may be NULL): labels outside [0, A) were met in the windows that meet
 *   [c0, c1), *n_bad of them.  Labels are only compared, never used as an index: such a haplotype counts for no ancestry at that window;
 *   the tables are as stated.
 * N == 0: nothing is launched, nothing is written.  Every form synchronises the context stream ONCE (the verdict on the labels, with the
 *   tables' copies of the host forms in front of it).  In the _dev form every pointer but n_bad is a device pointer.
 * gnx_ancestry_pair_counts_gt2: the file path's form.  G, n_variants, ldg, src as gnx_infer_gt2 takes them; labels (N, W) on the HOST,
 *   contiguous rows; the model's C, M, W and A.  A pair needs every row at once, so the WHOLE packed matrix is built in HBM, in device
 *   memory the call allocates and frees, batch by batch as gnx_ancestry_score_gt2 builds its batches, and the kernel runs once: the
 *   tables equal the matrix path's whatever GNX_HOST_BATCH is.  A model SNP the query lacks is missing in every row.  GNX_EUNSUPPORTED
 *   with the byte count in the message if the rows plus the tables exceed the device's memory; GNX_EINVAL before the launch also for a
 *   column map entry outside G. */
int gnx_ancestry_pair_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                 int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1,
                                 int32_t* d_DD, int32_t* d_DO, int32_t* d_OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad);
int gnx_ancestry_pair_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                             int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO,
                             int32_t* OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad);
int gnx_ancestry_pair_counts_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                                 const int32_t* labels, int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO, int32_t* OO,
                                 int64_t ld, int64_t* n_bad);

/* ---- ancestry-specific linkage disequilibrium on the int8 matrix cores (csrc/summary/k_ancestry_ld.hip) -------------------
 * INPUTS.  rows, row_kind, the codes, labels (N, W) int32, ld_rows, ld_labels, M, W, A, win(c) = min(c / M, W - 1) and the requirement
 *   M W <= C are EXACTLY gnx_ancestry_allele_counts'.  N need not be even: everything here is per haplotype.  For ONE ancestry
 *   `ancestry`, haplotype h and SNP c:
 *     o[h, c] = 1 if labels[h, win(c)] == ancestry AND the call is observed (code 0 or 1), else 0
 *     d[h, c] = 1 if o[h, c] and the code is 1, else 0
 * OUTPUTS.  Four int32 tables over the SNP range [c0, c1) and the offsets 0 <= k < band, of shape (c1 - c0, band), rows ld >= band ELEMENTS
 *   apart, OVERWRITTEN (the band columns of the c1 - c0 rows; what lies between band and ld is not touched); any may be NULL.  Entry
 *   [c - c0, k] speaks of the pair (c, c' = c + k) and is 0 where c + k >= C.  c + k may lie beyond c1: the tables of a partition of a
 *   range are the rows of the range's tables.
 *     n11 = sum_h d[h, c] d[h, c']     n1o = sum_h d[h, c] o[h, c']
 *     no1 = sum_h o[h, c] d[h, c']     noo = sum_h o[h, c] o[h, c']
 *   noo counts the haplotypes that carry the ancestry at BOTH SNPs (which may lie in different windows) with both calls observed, n1o and
 *   no1 the ALT calls at c and at c' among those, n11 the haplotypes ALT at both.  Every term is 0 or 1, so int32 is exact for every N the
 *   entry accepts.  All device arithmetic is integer: the tables depend on nothing but the inputs, not on the grid, the row form or the
 *   debug argument.  The caller derives r = (noo n11 - n1o no1) / sqrt(n1o (noo - n1o) no1 (noo - no1)) (gnomix_amd/ld.py).
 *   debug_haps_per_block: 0 in production (the split of the haplotypes over workgroups is taken from the number of tile pairs).  > 0
 *   (tests): the haplotypes one workgroup walks, rounded up to the kernel's chunk of 128.
 * GNX_EINVAL before any launch, nothing written: the conditions of gnx_ancestry_allele_counts (N < 0 or >= 2^31, C < 1, A < 1, M < 1,
 *   W < 1, M W > C, a stride too small, an unknown row_kind), ancestry outside [0, A), c0 < 0, c1 <= c0, c1 > C, band < 1, ld < band, a
 *   negative debug argument.
 * GNX_EUNSUPPORTED, nothing written: A > GNX_ALLELE_MAX_A, band > GNX_LD_MAX_BAND, more than 2^31 - 1 workgroups (tile pairs x haplotype
 *   segments).  GNX_LD_MAX_BAND is 4096: the kernel's layout sets no limit of its own (a band is walked in tiles of 64 SNPs, 66 of them
 *   at 4096), the bound keeps a table row at 16 KiB and a whole-chromosome call from asking for terabytes by a slip.
 * GNX_EINVAL after the launch, *n_bad set (0 otherwise; n_bad may be NULL): labels outside [0, A) were met in the windows of the SNPs
 *   c0 .. min(c1 - 1 + band - 1, C - 1), those the range AND its band reach, *n_bad of them.  Labels are only compared, never used as an
 *   index: such a haplotype counts for no ancestry at that window; the tables are as stated.
 * N == 0: nothing is launched, nothing is written.  Every form synchronises the context stream ONCE (the verdict on the labels, with the
 *   tables' copies of the host forms in front of it).  In the _dev form every pointer but n_bad is a device pointer.
 * gnx_ancestry_ld_counts_gt2: the file path's form.  G, n_variants, ldg, src as gnx_infer_gt2 takes them; labels (N, W) on the HOST,
 *   contiguous rows; the model's C, M, W and A.  The sums run over every row, so the WHOLE packed matrix is built in HBM, in device
 *   memory the call allocates and frees, batch by batch as gnx_ancestry_pair_counts_gt2 builds it, and the kernel runs once: the tables
 *   equal the matrix path's whatever GNX_HOST_BATCH is.  A model SNP the query lacks is missing in every row.  GNX_EUNSUPPORTED with the
 *   byte count in the message if the rows plus the tables exceed the device's memory; GNX_EINVAL before the launch also for a column map
 *   entry outside G.
 * OUT OF SCOPE: genotype (unphased) r^2, D', LD scores, pruning, several devices. */
#define GNX_LD_MAX_BAND 4096
int gnx_ancestry_ld_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                               int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band,
                               int32_t* d_n11, int32_t* d_n1o, int32_t* d_no1, int32_t* d_noo, int64_t ld, int64_t debug_haps_per_block,
                               int64_t* n_bad);
int gnx_ancestry_ld_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                           int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11,
                           int32_t* n1o, int32_t* no1, int32_t* noo, int64_t ld, int64_t debug_haps_per_block, int64_t* n_bad);
int gnx_ancestry_ld_counts_gt2(gnx_model* m, const uint8_t* G, int64_t n_variants, int64_t ldg, int64_t N, const int32_t* src,
                               const int32_t* labels, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11, int32_t* n1o,
                               int32_t* no1, int32_t* noo, int64_t ld, int64_t* n_bad);

/* per-kernel device time, measured with hipEvents on the context stream around every launch */
int gnx_profile_enable(gnx_ctx* ctx, int on);
int gnx_profile_reset(gnx_ctx* ctx);
int gnx_profile_get(gnx_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GNOMIX_HIP_H */
