"""Command-line surface of the reference's pre-trained mode (gnomix.py:318-355, 359-370, 404-412):

    python -m gnomix_amd <query_file> <output_basename> <chr_nr> <phase> <path_to_model>

`path_to_model` is a flat `.gnx` model (gnomix_amd.GnxModelData.save) or a reference `model.pkl[.gz]`, which is read
with a restricted unpickler (gnomix_amd.refpickle: neither the reference's `src` package nor xgboost is needed; CRF
models still need sklearn_crfsuite's attributes in the pickle) and converted by gnomix_amd.convert.from_reference_model.
Training mode (7-8 arguments, gnomix.py:158-306, 374-403):

    python -m gnomix_amd <query_file|None> <output_basename> <chr_nr> <phase> <genetic_map_file> <reference_file> <sample_map_file> [config.yaml]

simulates admixed haplotypes from the reference panel (gnomix_amd.simulate: draws on the host, matrix on the GPU), trains base and
smoother on the device (HipGnomix.train) and writes <output_basename>/models/<name>_chm_<chr>/<name>_chm_<chr>.gnx (a flat .gnx,
not the reference's pickled .pkl; it loads through the 5-argument form), analysis/confusion_matrix_{train,val}.txt and config.txt.
Mode "best" (CovRSK base, an SVC fit) is not built.  The extra config key model.smoother_kwargs (a dict) is passed to the smoother's
training (e.g. {max_ep: 20} for "large", {n_rounds: 50} for the default tree smoother).
Outputs: <output_basename>/query_results.msp, .fb (+ .lai, query_results_bed/, query_file_phased.vcf as configured).
"""
from __future__ import annotations

import os
import sys

import numpy as np

USAGE = ("Usage when training a model from scratch:\n"
         "   $ python3 gnomix.py <query_file> <output_basename> <chr_nr> <phase> <genetic_map_file> <reference_file> <sample_map_file> [config.yaml]\n"
         "Usage when using a pre-trained model:\n"
         "   $ python3 gnomix.py <query_file> <output_basename> <chr_nr> <phase> <path_to_model>")


PLANES_SUFFIX = ".planes"   # <model>.gnx.planes: the logistic base's prepared planes (DeviceModel.export_prepared), a cache


def read_gnx_and_planes(path):
    """the host half of loading a .gnx: the model file and, when present, the cache of its prepared planes -> (data, planes or None).
    Touches no GPU: the command line runs it on a worker thread while the main thread starts the GPU runtime."""
    from .model import GnxModelData
    data = GnxModelData.load(path)
    prepared = None
    side = path + PLANES_SUFFIX
    if os.environ.get("GNX_PLANES_CACHE", "1") != "0" and data.base_kind == "logistic" and os.path.exists(side):
        try:
            prepared = np.fromfile(side, dtype=np.uint8)
        except OSError as e:
            print("ignoring %s: %s" % (side, e), file=sys.stderr)
    return data, prepared


def _load_gnx_with_planes(path, device, verbose, timings=None, file_job=None):
    """A .gnx and, beside it, the cache of its prepared planes (<model>.gnx.planes).  Starting the GPU runtime is the largest part
    of a cold start (0.13-0.2 s of hipInit) and needs nothing of the model: the file reads run on a worker thread meanwhile
    (`file_job`, started by main() before it first touches the GPU).  A cache that does not belong to the model / library / settings
    is reported, ignored and rewritten.  GNX_PLANES_CACHE=0: neither read nor written."""
    from time import perf_counter as clock
    from . import _lib
    from .gnomix import HipGnomix
    t0 = clock()
    if file_job is None:
        file_job = _Prefetch(lambda: read_gnx_and_planes(path))
    ctx = _lib.default_context(device)
    t1 = clock()
    data, prepared = file_job.result()
    use_cache = os.environ.get("GNX_PLANES_CACHE", "1") != "0" and data.base_kind == "logistic"
    side = path + PLANES_SUFFIX
    t2 = clock()
    model = None
    if prepared is not None:
        try:
            model = HipGnomix(data, ctx=ctx, prepared=prepared)
        except _lib.GnxError as e:
            if e.code != _lib.GNX_ESTALE:
                raise
            print("%s is stale (%s): preparing the planes from the model and rewriting it" % (side, e.msg), file=sys.stderr)
            prepared = None
    if model is None:
        model = HipGnomix(data, ctx=ctx)
        if use_cache:
            try:
                blob = model.dev.export_prepared()
                if blob.size:
                    tmp = "%s.tmp%d" % (side, os.getpid())
                    blob.tofile(tmp)
                    os.replace(tmp, side)      # (atomic: a concurrent start reads the old file or the new one, never half of it)
            except OSError as e:               # a read-only model directory: every start prepares the planes, as before
                if verbose:
                    print("not caching the prepared planes (%s)" % e, file=sys.stderr)
    if timings is not None:
        timings.update({"load_model.gpu_runtime": t1 - t0, "load_model.wait_file": t2 - t1, "load_model.device_model": clock() - t2,
                        "load_model.planes_from_cache": float(prepared is not None)})
    return model


def load_model(path_to_model, device=0, verbose=True, timings=None, file_job=None):
    """gnomix.py:26-35 — .gnx directly, .pkl / .pkl.gz through the converter"""
    from .gnomix import HipGnomix
    if verbose:
        print("Loading model...")
    if path_to_model.endswith(".gnx"):
        return _load_gnx_with_planes(path_to_model, device, verbose, timings, file_job)
    from .convert import from_reference_model
    from .refpickle import load_reference_pickle
    # restricted unpickling: the reference's `src` package and xgboost are NOT needed (and nothing of them is executed)
    try:
        ref_model = load_reference_pickle(path_to_model)
    except Exception as e:   # e.g. estimators pickled by an incompatible scikit-learn: fall back to attribute bags
        if verbose:
            print("rebuilding scikit-learn objects failed (%s): reading their attributes only" % type(e).__name__)
        ref_model = load_reference_pickle(path_to_model, use_sklearn=False)
    return HipGnomix(from_reference_model(ref_model), device=device)


class _Prefetch:
    """`fn()` on a worker thread (the library calls release the GIL); result() re-raises what it raised"""

    def __init__(self, fn):
        import threading
        self._out = self._err = None

        def work():
            try:
                self._out = fn()
            except BaseException as e:   # noqa: BLE001 - handed to the caller
                self._err = e
        self._t = threading.Thread(target=work, daemon=True)
        self._t.start()

    def result(self):
        self._t.join()
        if self._err is not None:
            raise self._err
        return self._out


def run_inference(base_args, model, snp_level=False, bed_file_output=False, verbose=False, timings=None, query=None, devices=None,
                  global_ancestry_output=False, ancestry_allele_freq_output=False, ancestry_assoc_output=False, phenotype_file=None,
                  ancestry_assoc_model="linear", ancestry_score_output=False, score_file=None, ancestry_mds_output=False,
                  ancestry_mds_components=None, ancestry_mds_min_sites=None, ancestry_clump_output=False, ancestry_clump_p1=None,
                  ancestry_clump_p2=None, ancestry_clump_r2=None, ancestry_clump_kb=None, trait_file=None, covariate_file=None,
                  admixture_mapping_output=False, admixture_mapping_perms=None, admixture_mapping_seed=None, admixture_mapping_min_hap=None):
    """gnomix.py:37-100 with the HIP model behind the same steps.  The query never becomes an (N, C) host matrix: the library
    parses the text into 2-bit rows (gnx_vcf_read), `column_map` keeps vcf_to_npy's bookkeeping (SNP intersection, REF flips,
    absent SNPs) as one int32 per model SNP, the GPU builds X and runs base + smoother (or Gnofix) on it, and the library
    formats .msp / .fb / the phased VCF.  `timings` (a dict) receives the seconds of each stage; `query` = a _Prefetch of
    vcfio.read_vcf started earlier (the command line parses the query while the GPU runtime starts and the model loads).
    `devices` = GPU ordinals (several: the individuals are cut over them, one context and one host thread each, the query parsed
    once and the outputs written once: gnomix_amd/multi.py) or an existing multi.DeviceGroup; None = the model's own device.
    `global_ancestry_output` (config key inference.global_ancestry_output, off unless set): query_results.Q (global ancestry per
    individual, hard calls) and query_results.tracts.tsv (tract statistics per haplotype and ancestry) as well, both with cM weights,
    from the labels the .msp gets (Gnofix's when phasing), summarised on the device (gnx_ancestry_summary).
    `ancestry_allele_freq_output` (config key inference.ancestry_allele_freq_output, off unless set): query_results.afreq.tsv as well,
    the ancestry-specific allele counts and frequencies of every model SNP, counted on the device from the query's 2-bit rows and the
    labels the .msp gets (gnx_ancestry_allele_counts_gt2).  Not with phase=True (ValueError before any work): the phased matrix is not
    kept on that path; HipGnomix.phase followed by HipGnomix.allele_frequencies covers that use.
    `ancestry_assoc_output` (config key inference.ancestry_assoc_output, off unless set) with `phenotype_file` (inference.phenotype_file:
    a TSV with the header `sample  pheno  [covariates]`, matched by sample name; query samples it lacks take no part; an intercept is
    added): query_results.assoc.tsv as well, the ancestry-specific association (Tractor model) of every model
    SNP, its statistics reduced on the model's own GPU from the query's 2-bit rows and the labels the .msp gets
    (gnx_ancestry_assoc_stats_gt2).  Not with phase=True (ValueError before any work), for the same reason.
    `ancestry_assoc_model` (config key inference.ancestry_assoc_model: linear | logistic; absent = linear): with logistic the
    phenotype is a case / control trait coded 0 / 1 (another value on a used sample: ValueError naming the sample) and the file is
    query_results.assoc.logistic.tsv instead, one logistic fit per SNP on the device (gnx_ancestry_assoc_logit_gt2).
    `trait_file` (config key inference.trait_file: a TSV with the header `sample  name...`, one column per quantitative trait, matched by
    sample name; a query sample it lacks takes no part) with ancestry_assoc_output, and optionally `covariate_file`
    (inference.covariate_file: header `sample  cov...`; an intercept is added): one query_results.assoc.<name>.tsv per trait, in
    write_assoc's format, all traits fitted at once chunk of SNPs by chunk (gnx_ancestry_assoc_traits_gt2, DESIGN.md section 4.23;
    complete cases across the traits) and appended chunk by chunk.  It takes the place of phenotype_file (both may be given); linear
    model only; not with phase=True (the ValueError above); clumping needs phenotype_file.
    `ancestry_score_output` (config key inference.ancestry_score_output, off unless set) with `score_file` (inference.score_file: a TSV
    with the header `chm  pos  effect_allele` and weight columns NAME or NAME:POP, score.read_score_file): query_results.sscore.tsv as
    well, the ancestry-partitioned polygenic scores of every individual, summed on the model's own GPU from the query's 2-bit rows
    and the labels the .msp gets (gnx_ancestry_score_gt2).  Not with phase=True (ValueError before any work), for the
    same reason.
    `ancestry_mds_output` (config key inference.ancestry_mds_output, off unless set; inference.ancestry_mds_components, default 4, and
    inference.ancestry_mds_min_sites, default 1000, optional): query_results.asmds.tsv as well, the ancestry-specific MDS of every
    ancestry: the pair count tables from the model's own GPU, from the query's 2-bit rows and the labels the .msp gets
    (gnx_ancestry_pair_counts_gt2), the embedding on the host (gnomix_amd.asmds).  An ancestry with fewer than
    components + 1 individuals kept gets a header line and no rows.  Not with phase=True (ValueError before any work), for the same
    reason.
    `ancestry_clump_output` (config key inference.ancestry_clump_output, off unless set; it needs ancestry_assoc_output; optional
    inference.ancestry_clump_p1, _p2, _r2, _kb, defaults 1e-4, 1e-2, 0.5, 250): query_results.clumped.tsv as well, the association
    result clumped ancestry by ancestry (gnomix_amd.ld.clump) with that ancestry's LD, counted on the model's own GPU from the query's
    2-bit rows and the labels the .msp gets (gnx_ancestry_ld_counts_gt2).  Not with phase=True (ValueError before any
    work), for the same reason.
    `admixture_mapping_output` (config key inference.admixture_mapping_output, off unless set) with `phenotype_file` or `trait_file`
    (plus `covariate_file`), read as above: admixture mapping, the regression of the trait(s) on the local ancestry itself window by
    window (gnx_ancestry_admixmap), from the labels the .msp gets: query_results.admixmap.tsv for phenotype_file,
    query_results.admixmap.<name>.tsv per trait of trait_file (postprocess.write_admixmap).  inference.admixture_mapping_perms (default
    0: no permutations), _seed (default 0) and _min_hap (default 1) go to admixmap.admixture_mapping.  No genotypes are needed, so it
    works with phase False AND True (Gnofix's labels then).  A missing file or a bad value is a ValueError before any work."""
    from time import perf_counter as clock
    from . import postprocess as pp
    from . import vcfio
    if ancestry_clump_output and base_args["phase"]:
        raise ValueError("inference.ancestry_clump_output with phase=True: the phased haplotypes are not kept on this path; "
                         "use HipGnomix.phase followed by HipGnomix.ancestry_association and HipGnomix.ancestry_clump")
    if ancestry_clump_output and not ancestry_assoc_output:
        raise ValueError("inference.ancestry_clump_output needs inference.ancestry_assoc_output (the p-values it clumps)")
    clump_kw = {k: float(v) for k, v in (("p1", ancestry_clump_p1), ("p2", ancestry_clump_p2), ("r2", ancestry_clump_r2),
                                         ("kb", ancestry_clump_kb)) if v is not None}
    if ancestry_allele_freq_output and base_args["phase"]:
        raise ValueError("inference.ancestry_allele_freq_output with phase=True: the phased haplotypes are not kept on this path; "
                         "use HipGnomix.phase followed by HipGnomix.allele_frequencies")
    if ancestry_assoc_model not in ("linear", "logistic"):
        raise ValueError(f"inference.ancestry_assoc_model must be 'linear' or 'logistic', got {ancestry_assoc_model!r}")
    if ancestry_assoc_output and base_args["phase"]:
        raise ValueError("inference.ancestry_assoc_output with phase=True: the phased haplotypes are not kept on this path; "
                         "use HipGnomix.phase followed by HipGnomix.ancestry_association")
    if ancestry_assoc_output and not phenotype_file and not trait_file:
        raise ValueError("inference.ancestry_assoc_output needs inference.phenotype_file (a TSV: sample, pheno, then covariates)")
    if ancestry_assoc_output and trait_file and ancestry_assoc_model != "linear":
        raise ValueError("inference.trait_file: several traits at once are fitted with inference.ancestry_assoc_model linear only")
    if ancestry_clump_output and not phenotype_file:
        raise ValueError("inference.ancestry_clump_output clumps the result of inference.phenotype_file, not those of inference.trait_file")
    if covariate_file and not trait_file:
        raise ValueError("inference.covariate_file goes with inference.trait_file (inference.phenotype_file carries its own covariates)")
    if ancestry_score_output and base_args["phase"]:
        raise ValueError("inference.ancestry_score_output with phase=True: the phased haplotypes are not kept on this path; "
                         "use HipGnomix.phase followed by HipGnomix.ancestry_scores")
    if ancestry_score_output and not score_file:
        raise ValueError("inference.ancestry_score_output needs inference.score_file (a TSV: chm, pos, effect_allele, then weight columns)")
    if ancestry_mds_output and base_args["phase"]:
        raise ValueError("inference.ancestry_mds_output with phase=True: the phased haplotypes are not kept on this path; "
                         "use HipGnomix.phase followed by HipGnomix.ancestry_mds")
    am_perms = 0 if admixture_mapping_perms is None else int(admixture_mapping_perms)
    am_seed = 0 if admixture_mapping_seed is None else int(admixture_mapping_seed)
    am_min_hap = 1 if admixture_mapping_min_hap is None else int(admixture_mapping_min_hap)
    if admixture_mapping_output:
        if not phenotype_file and not trait_file:
            raise ValueError("inference.admixture_mapping_output needs inference.phenotype_file (a TSV: sample, pheno, then covariates) or "
                             "inference.trait_file")
        for key, path in (("phenotype_file", phenotype_file), ("trait_file", trait_file), ("covariate_file", covariate_file)):
            if path and not os.path.isfile(path):
                raise ValueError(f"inference.{key}: no such file: {path}")
        if am_perms < 0:
            raise ValueError("inference.admixture_mapping_perms must be >= 0")
        if am_min_hap < 1:
            raise ValueError("inference.admixture_mapping_min_hap must be >= 1")
    mds_k = 4 if ancestry_mds_components is None else int(ancestry_mds_components)
    mds_sites = 1000 if ancestry_mds_min_sites is None else int(ancestry_mds_min_sites)
    if ancestry_mds_output and (mds_k < 1 or mds_sites < 1):
        raise ValueError("inference.ancestry_mds_components and inference.ancestry_mds_min_sites must be >= 1")
    query_file, chm, output_path = base_args["query_file"], base_args["chm"], base_args["output_basename"]
    T = timings if timings is not None else {}
    if verbose:
        print("Loading and processing query file...")
    t0 = clock()
    vcf = query.result() if query is not None else vcfio.read_vcf(query_file, chm=chm, ctx=model.dev.ctx)
    assert vcf is not None, "No SNPs of specified chromosome found in query file."
    T["read_vcf"] = clock() - t0
    t0 = clock()
    src, vcf_idx, fmt_idx = vcfio.column_map(vcf, model.snp_pos, model.snp_ref, verbose=verbose)
    N = 2 * vcf.n_samples
    T["column_map"] = clock() - t0
    if verbose:
        print("Inferring ancestry on query data...")
    t0 = clock()
    out = (model.dev.ctx.pinned_empty((N, model.W, model.A), model.dev.proba_dtype()), model.dev.ctx.pinned_empty((N, model.W), np.int32))
    runner = model.dev
    own_group = None
    if devices is not None and not isinstance(devices, (list, tuple)):
        runner = devices                                                   # a DeviceGroup the caller keeps
    elif devices is not None and len(devices) > 1 and vcf.n_samples > 1:
        from .multi import DeviceGroup
        # no more replicas than shards of whole individuals; made on one thread per device; released below whatever happens
        own_group = DeviceGroup(model.data, devices, first=model.dev, n_ind=vcf.n_samples)
        if len(own_group.models) > 1:
            runner = own_group
        T["replicate_model"] = clock() - t0
        t0 = clock()
    try:
        return _run_and_write(model, base_args, runner, vcf, src, vcf_idx, fmt_idx, N, out, T, t0, snp_level, bed_file_output, verbose,
                              global_ancestry_output, ancestry_allele_freq_output, ancestry_assoc_output, phenotype_file, ancestry_assoc_model,
                              ancestry_score_output=ancestry_score_output, score_file=score_file,
                              ancestry_mds=(mds_k, mds_sites) if ancestry_mds_output else None,
                              ancestry_clump=clump_kw if ancestry_clump_output else None, trait_file=trait_file, covariate_file=covariate_file,
                              admixture_mapping=(am_perms, am_seed, am_min_hap) if admixture_mapping_output else None)
    finally:
        if own_group is not None:
            own_group.close()


def _run_and_write(model, base_args, runner, vcf, src, vcf_idx, fmt_idx, N, out, T, t0, snp_level, bed_file_output, verbose,
                   global_ancestry_output=False, ancestry_allele_freq_output=False, ancestry_assoc_output=False, phenotype_file=None,
                   ancestry_assoc_model="linear", ancestry_score_output=False, score_file=None, ancestry_mds=None, ancestry_clump=None,
                   trait_file=None, covariate_file=None, admixture_mapping=None):
    from time import perf_counter as clock
    from . import postprocess as pp
    from . import vcfio
    chm, output_path = base_args["chm"], base_args["output_basename"]
    mode_filter = getattr(model.smooth, "mode_filter", 0) if model.smooth is not None else 0
    if not base_args["phase"]:
        proba, labels = runner.infer_gt2(vcf.gt2, N, src, out=out)
        if mode_filter:   # Smoother.predict's filter: the .msp labels (and .lai / .bed) are filtered, the .fb probabilities are not
            labels = model.dev.mode_filter(labels, mode_filter)
        T["infer"] = clock() - t0
    else:
        if mode_filter:
            raise NotImplementedError("phase with mode_filter != 0: the filter inside the Gnofix loop is not built")
        assert model.smooth is not None, "Smoother is not trained, returning original haplotypes"
        assert model.smooth.gnofix, "Type of Smoother ({}) does not currently support re-phasing".format(model.smooth)
        G_phased, proba, labels, _ = runner.phase_gt2(vcf.gt2, N, src, out_cols=fmt_idx, out=out)
        T["phase"] = clock() - t0
        if verbose:
            print("Writing phased SNPs to disk...")
        t0 = clock()
        rows = np.asarray(vcf_idx) if vcf.rows is None else np.asarray(vcf.rows)[vcf_idx]
        vcfio.write_phased_vcf(vcf, rows, G_phased, output_path + "/" + "query_file_phased", ref=np.asarray(model.snp_ref)[fmt_idx],
                               alt=np.asarray(model.snp_alt)[fmt_idx], headers=vcf.meta_header)
        T["write_vcf"] = clock() - t0
    if verbose:
        print("Saving results...")
    t0 = clock()
    gm_pos, gm_cm = model.data.gen_map_pos, model.data.gen_map_cm
    meta = pp.get_meta_data(chm, model.snp_pos, vcf["variants/POS"], model.W, model.M, gm_pos, gm_cm)
    out_prefix = output_path + "/" + "query_results"
    samples = vcf["samples"]
    pp.write_msp(out_prefix, meta, labels, model.population_order, samples)
    T["write_msp"] = clock() - t0
    t0 = clock()
    pp.write_fb(out_prefix, meta, proba, model.population_order, samples, ctx=model.dev.ctx if os.environ.get("GNX_FB_DEV") == "1" else None)
    T["write_fb"] = clock() - t0
    # (.lai and .bed from the labels held here: the same bytes as postprocess.msp_to_lai / msp_to_bed make from the .msp text)
    if snp_level:
        t0 = clock()
        pp.write_lai(out_prefix, meta, labels, vcf["variants/POS"], samples, populations=model.population_order)
        T["write_lai"] = clock() - t0
    if bed_file_output:
        t0 = clock()
        pp.write_bed(output_path + "/" + "query_results_bed", meta, labels, samples, pop_order=model.population_order, ctx=model.dev.ctx)
        T["write_bed"] = clock() - t0
    if global_ancestry_output:
        t0 = clock()
        summary = runner.ancestry_summary(labels, pp.window_weights(meta, "cM"))
        pp.write_q(out_prefix, summary.hard, model.population_order, samples)
        pp.write_tracts(out_prefix, summary, model.population_order, samples)
        T["write_global_ancestry"] = clock() - t0
    if ancestry_allele_freq_output:
        t0 = clock()
        counts = runner.allele_counts_gt2(vcf.gt2, N, src, labels)
        pp.write_afreq(out_prefix, chm, model.snp_pos, model.M, model.W, counts, model.population_order)
        T["write_afreq"] = clock() - t0
    if admixture_mapping is not None:
        t0 = clock()
        from . import admixmap, assoc
        n_perm, seed, min_hap = admixture_mapping
        names = [str(s) for s in samples]
        lab32 = np.ascontiguousarray(labels, dtype=np.int32)
        if trait_file:
            Y, Z, use, trait_names, _ = assoc.read_traits(trait_file, names, covariate_file)
            for name in trait_names:
                if not name or os.sep in name or name in (".", ".."):
                    raise ValueError(f"{trait_file}: the trait name '{name}' cannot be part of a file name")
            res = admixmap.admixture_mapping(model.dev.ctx, lab32, model.A, Y, Z, use, min_hap, n_perm, seed)     # one GPU: the model's own
            pp.write_admixmap(out_prefix, meta, res, model.population_order, trait_names)
        if phenotype_file:
            y, Z, use, _ = assoc.read_phenotypes(phenotype_file, names)
            res = admixmap.admixture_mapping(model.dev.ctx, lab32, model.A, y, Z, use, min_hap, n_perm, seed)
            pp.write_admixmap(out_prefix, meta, res, model.population_order)
        T["write_admixmap"] = clock() - t0
    if ancestry_assoc_output and trait_file:
        t0 = clock()
        from . import assoc
        Y, Z, use, trait_names, _ = assoc.read_traits(trait_file, [str(s) for s in samples], covariate_file)
        for name in trait_names:
            if not name or os.sep in name or name in (".", ".."):
                raise ValueError(f"{trait_file}: the trait name '{name}' cannot be part of a file name")
        for c0, c1, res in model.dev.ancestry_assoc_traits_gt2_chunks(vcf.gt2, N, src, labels, Y, Z, use):     # one GPU: the model's own
            for t, name in enumerate(trait_names):
                one = assoc.AncestryAssoc(res.beta[:, :, t], res.se[:, :, t], res.t[:, :, t], res.p[:, :, t], res.n_alt, res.n_hap, res.n, res.df,
                                          res.n_miss, res.status)
                pp.write_assoc(out_prefix, chm, model.snp_pos, model.M, model.W, one, model.population_order, c0=c0, name=name)
        T["write_assoc_traits"] = clock() - t0
    if ancestry_assoc_output and phenotype_file:
        t0 = clock()
        from . import assoc
        names = [str(s) for s in samples]
        y, Z, use, _ = assoc.read_phenotypes(phenotype_file, names)
        if ancestry_assoc_model == "logistic":
            assoc.check_binary(y, use, names)
            result = model.dev.ancestry_assoc_logit_gt2(vcf.gt2, N, src, labels, y, Z, use)
            pp.write_assoc_logit(out_prefix, chm, model.snp_pos, model.M, model.W, result, model.population_order)
        else:
            result = model.dev.ancestry_assoc_gt2(vcf.gt2, N, src, labels, y, Z, use)     # one GPU: the model's own
            pp.write_assoc(out_prefix, chm, model.snp_pos, model.M, model.W, result, model.population_order)
        T["write_assoc"] = clock() - t0
        if ancestry_clump is not None:
            t0 = clock()
            from . import ld
            pos = np.asarray(model.snp_pos).astype(np.int64)
            band = ld.band_for(pos, ancestry_clump.get("kb", 250))
            pv = np.asarray(result.p, dtype=np.float64)
            index_of = np.full(pv.shape, -1, np.int64)
            for a in range(model.A):                                                              # one GPU: the model's own
                fetch = lambda c0, c1, a=a: model.dev.ancestry_ld_counts_gt2(vcf.gt2, N, src, labels, a, c0, c1, band)
                index_of[:, a] = ld.clump(pv[:, a], pos, ld.BlockCache(fetch, model.C, max(4096, 4 * band)), **ancestry_clump)
            pp.write_clumps(out_prefix, chm, model.snp_pos, index_of, pv, model.population_order)
            T["write_clumps"] = clock() - t0
    if ancestry_score_output:
        t0 = clock()
        from . import score
        weights, effect, names, _ = score.read_score_file(score_file, chm, model.snp_pos, model.snp_ref, model.snp_alt, model.population_order)
        result = model.dev.ancestry_scores_gt2(vcf.gt2, N, src, labels, weights, effect)         # one GPU: the model's own
        pp.write_sscore(out_prefix, result, names, model.population_order, [str(s) for s in samples])
        T["write_sscore"] = clock() - t0
    if ancestry_mds is not None:
        t0 = clock()
        from . import asmds
        k, min_sites = ancestry_mds
        results = [asmds.ancestry_mds(model.dev.ancestry_pair_counts_gt2(vcf.gt2, N, src, labels, a), k=k, min_sites=min_sites)
                   for a in range(model.A)]                                                      # one GPU: the model's own
        pp.write_asmds(out_prefix, results, model.population_order, [str(s) for s in samples])
        T["write_asmds"] = clock() - t0
    return out_prefix


def _since_process_start():
    """seconds since this process was created (Linux: /proc/self/stat field 22 against /proc/uptime)"""
    try:
        with open("/proc/self/stat") as f:
            start_ticks = float(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/uptime") as f:
            up = float(f.read().split()[0])
        return up - start_ticks / os.sysconf("SC_CLK_TCK")
    except Exception:
        return float("nan")


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    t_startup = _since_process_start() if os.environ.get("GNX_CLI_TIMING") else None
    if len(argv) in (8, 9):
        return train_main(argv)   # (decides about torch itself: the device-resident training path hands it tensors)
    if "torch" not in sys.modules:
        os.environ.setdefault("GNX_NO_TORCH", "1")   # the command line needs no torch: do not pay for its import
    if len(argv) != 6:
        if len(argv) > 1:
            print("Error: Incorrect number of arguments.")
        print(USAGE)
        return 0
    base_args = {"mode": "pre-trained", "query_file": argv[1] if argv[1].strip() != "None" else None,
                 "output_basename": argv[2], "chm": argv[3], "phase": argv[4].lower() == "true", "path_to_model": argv[5]}
    os.makedirs(base_args["output_basename"], exist_ok=True)
    config = {"model": {}, "inference": {}}
    if os.path.exists("./config.yaml"):
        import yaml
        with open("./config.yaml") as f:
            config = yaml.safe_load(f) or config
    print("Launching in pre-trained mode...")
    from time import perf_counter as clock
    query = None
    if base_args["query_file"] and os.environ.get("GNX_CLI_PREFETCH", "1") != "0":
        # neither needs the other: the host's threads parse the text (into pageable memory, no GPU context yet) while this
        # thread starts the GPU runtime (~0.16 s), reads the model and builds its device tables (~0.15 s)
        from . import vcfio
        query = _Prefetch(lambda: vcfio.read_vcf(base_args["query_file"], chm=base_args["chm"], ctx=None))
    t_load = clock()
    file_job, T_load = None, {}
    if base_args["path_to_model"].endswith(".gnx"):   # the model file is read beside the GPU runtime's start (visible_devices is its first use)
        mp = base_args["path_to_model"]
        file_job = _Prefetch(lambda: read_gnx_and_planes(mp))
    from .multi import visible_devices
    devices = visible_devices()        # every GPU of the node (GNX_DEVICES="0,1,.." narrows it): individuals are cut over them
    model = load_model(base_args["path_to_model"], device=devices[0], timings=T_load, file_job=file_job)
    t_load = clock() - t_load
    model.n_cores = (config.get("model") or {}).get("n_cores")            # gnomix.py:365-367
    model.calibrate = (config.get("model") or {}).get("calibrate")
    model.smooth.calibrate = model.calibrate
    model.base.vectorize = True                                           # gnomix.py:370
    if base_args["query_file"]:
        print("Launching inference...")
        inf = config.get("inference") or {}
        T = {"load_model": t_load}
        if t_startup is not None:
            T = {"interpreter_and_imports": t_startup, "load_model": t_load}
        T.update(T_load)
        run_inference(base_args, model, snp_level=bool(inf.get("snp_level_inference")),
                      bed_file_output=bool(inf.get("bed_file_output")), verbose=True, timings=T, query=query, devices=devices,
                      global_ancestry_output=bool(inf.get("global_ancestry_output")),
                      ancestry_allele_freq_output=bool(inf.get("ancestry_allele_freq_output")),
                      ancestry_assoc_output=bool(inf.get("ancestry_assoc_output")), phenotype_file=inf.get("phenotype_file"),
                      ancestry_assoc_model=inf.get("ancestry_assoc_model") or "linear",
                      ancestry_score_output=bool(inf.get("ancestry_score_output")), score_file=inf.get("score_file"),
                      ancestry_mds_output=bool(inf.get("ancestry_mds_output")), ancestry_mds_components=inf.get("ancestry_mds_components"),
                      ancestry_mds_min_sites=inf.get("ancestry_mds_min_sites"),
                      ancestry_clump_output=bool(inf.get("ancestry_clump_output")), ancestry_clump_p1=inf.get("ancestry_clump_p1"),
                      ancestry_clump_p2=inf.get("ancestry_clump_p2"), ancestry_clump_r2=inf.get("ancestry_clump_r2"),
                      ancestry_clump_kb=inf.get("ancestry_clump_kb"), trait_file=inf.get("trait_file"),
                      covariate_file=inf.get("covariate_file"), admixture_mapping_output=bool(inf.get("admixture_mapping_output")),
                      admixture_mapping_perms=inf.get("admixture_mapping_perms"), admixture_mapping_seed=inf.get("admixture_mapping_seed"),
                      admixture_mapping_min_hap=inf.get("admixture_mapping_min_hap"))
        if os.environ.get("GNX_CLI_TIMING"):
            T["since_process_start"] = _since_process_start()
            sys.stderr.write("gnomix_amd timings (s): " + ", ".join("%s %.3f" % kv for kv in T.items()) + "\n")
    return 0


def training_setup(argv):
    """the host half of training mode up to the first device call: arguments, config (the reference's defaults under the file's
    values), the checks the reference makes (gnomix.py:335-389) -> (base_args, config, error message or None)"""
    base_args = {"mode": "train", "query_file": argv[1] if argv[1].strip() != "None" else None, "output_basename": argv[2],
                 "chm": argv[3], "phase": argv[4].lower() == "true", "genetic_map_file": argv[5], "reference_file": argv[6],
                 "sample_map_file": argv[7], "config_file": argv[8] if len(argv) == 9 else "./config.yaml"}
    from .simulate import merge_config
    user = {}
    if len(argv) == 9 or os.path.exists(base_args["config_file"]):
        if not os.path.exists(base_args["config_file"]):
            return base_args, None, "config file %s not found" % base_args["config_file"]
        import yaml
        with open(base_args["config_file"]) as f:
            user = yaml.safe_load(f) or {}
    config = merge_config(user)
    sim = config["simulation"]
    mode = config["model"].get("inference") or "default"
    if mode == "best":
        return base_args, config, ('model mode "best" (CovRSK base, an SVC fit per window) cannot be trained by this build: '
                                   'use "default", "fast" or "large"')
    if mode not in ("default", "fast", "large"):
        return base_args, config, "unknown model mode %r" % mode
    from_path = sim.get("run") is False and sim.get("path") is not None
    need = ["genetic_map_file"] + ([] if from_path else ["reference_file", "sample_map_file"])
    for k in need:
        if not os.path.isfile(base_args[k]):
            return base_args, config, "%s %s not found" % (k.replace("_", " "), base_args[k])
    if from_path and not os.path.isfile(os.path.join(sim["path"], "metadata.pkl")):
        return base_args, config, "no simulated data at %s (metadata.pkl missing)" % sim["path"]
    if base_args["query_file"] and not os.path.isfile(base_args["query_file"]):
        return base_args, config, "query file %s not found" % base_args["query_file"]
    return base_args, config, None


def train_resident(config, environ=None):
    """whether training mode simulates into HBM and trains from there (SimPlan.materialise_dev + the CUDA-tensor form of
    HipGnomix.train): mode "default" (the logistic base with the tree smoother: the pair that trains without leaving the device),
    data that are simulated now (not read from simulation.path) and NOT kept (simulation.rm_data: generated data that must be
    written to <output>/generated_data are host arrays anyway), torch importable, and neither GNX_TRAIN_RESIDENT=0 nor
    GNX_NO_TORCH set"""
    environ = os.environ if environ is None else environ
    sim, mode = config["simulation"], config["model"].get("inference") or "default"
    if environ.get("GNX_TRAIN_RESIDENT", "1") == "0" or environ.get("GNX_NO_TORCH"):
        return False
    if mode != "default" or not sim.get("rm_data") or (sim.get("run") is False and sim.get("path") is not None):
        return False
    import importlib.util
    return importlib.util.find_spec("torch") is not None


def _initial_model(C, M, A, S, context, mode, seed, meta):
    """an untrained model of the mode's kinds (gnomix_amd.train.untrained_model)"""
    from .train import untrained_model
    return untrained_model(C, M, A, S, context, mode, seed=seed, meta=meta)


def write_model_config(model, path):
    """what Gnomix.write_config (src/model.py) means to write: every public int / float / str / bool attribute, one per line"""
    with open(path, "w") as f:
        for attr in sorted(vars(model)):
            val = getattr(model, attr)
            if not attr.startswith("_") and isinstance(val, (int, float, str, bool, np.integer, np.floating)):
                f.write("{}\t{}\n".format(attr, val))


def train_main(argv):
    """gnomix.py:372-403 (simulate_splits, train_model) and, with a query, run_inference on the model just trained"""
    base_args, config, err = training_setup(argv)
    if err:
        print("Error: " + err)
        return 2
    from time import perf_counter as clock
    resident = train_resident(config)
    if resident:
        import torch  # noqa: F401  (before the library is loaded: both then share one HIP runtime, gnomix_amd/_lib.py)
    elif "torch" not in sys.modules:
        os.environ.setdefault("GNX_NO_TORCH", "1")   # the host-array path needs no torch: do not pay for its import
    from . import simulate as sim_mod
    from . import _lib
    from .gnomix import HipGnomix
    print("Launching in training mode...")
    verbose = bool(config.get("verbose"))
    sim, mcfg, chm = config["simulation"], config["model"], base_args["chm"]
    out = base_args["output_basename"]
    os.makedirs(out, exist_ok=True)
    gmap = sim_mod.read_genetic_map(base_args["genetic_map_file"], chm)
    T = {}
    t0 = clock()
    if sim.get("run") is False and sim.get("path") is not None:
        print("Using pre-simulated data from: ", sim["path"])
        ratios = {k: v for k, v in sim["splits"]["ratios"].items() if not (k == "val" and v == 0)}
        gens = {k: v for k, v in sim_mod.split_generations(sim).items() if k in ratios}
        data, meta = sim_mod.read_generated_data(sim["path"], gens, mcfg["window_size_cM"])
        C, M, A = meta["C"], meta["M"], meta["A"]
        ctx = _lib.default_context(0)
        T["read_data"] = clock() - t0
    else:
        try:
            plan = sim_mod.plan_splits(base_args["reference_file"], gmap, base_args["sample_map_file"], config, chm=chm, verbose=False)
        except ValueError as e:
            print("Error: %s" % e)
            return 2
        T["plan"] = clock() - t0
        C, A = plan.C, plan.A
        M = plan.window_size(mcfg["window_size_cM"])
        meta = {"snp_pos": plan.meta["pos_snps"], "snp_ref": plan.meta["ref_snps"], "snp_alt": plan.meta["alt_snps"], "pop_order": plan.pop_order}
        if verbose:
            print("Running Simulation...")
        t0 = clock()
        ctx = _lib.default_context(0)
        keep = not sim.get("rm_data")
        if resident:   # (implies not keep) the splits are built in HBM and stay there: HipGnomix.train reads them in place
            data, anc = plan.materialise_dev(ctx, M=M), None
        else:
            (data, anc) = plan.materialise(ctx, M=M, want_anc=True) if keep else (plan.materialise(ctx, M=M), None)
        T["simulate_dev" if resident else "simulate"] = clock() - t0
        if keep:
            t0 = clock()
            X_all = np.concatenate([d[0] for d in data if d[0] is not None])
            sim_mod.write_generated_data(plan, os.path.join(out, "generated_data"), X_all, anc, gen_map=gmap)
            del X_all, anc
            T["write_data"] = clock() - t0
    mode = mcfg.get("inference") or "default"
    context = int(M * mcfg["context_ratio"])
    d = _initial_model(C, M, A, int(mcfg["smooth_size"]), context, mode, config["seed"], meta)
    d.gen_map_pos, d.gen_map_cm = gmap["pos"].to_numpy(np.int64), gmap["pos_cm"].to_numpy(np.float64)
    model = HipGnomix(d, ctx=ctx, calibrate=bool(mcfg.get("calibrate")))
    kw = dict(mcfg.get("smoother_kwargs") or {})
    if mode == "large":
        kw.setdefault("seed", config["seed"])
    if verbose:
        print("Building model...")
    t0 = clock()
    model.train(data=data, retrain_base=bool(mcfg.get("retrain_base")), evaluate=True, verbose=verbose, **kw)
    T["train"] = clock() - t0
    validate = data[2][0] is not None
    name = mcfg.get("name") or "model"
    repo = os.path.join(out, "models", "%s_chm_%s" % (name, chm))
    os.makedirs(os.path.join(repo, "analysis"), exist_ok=True)
    model.save(os.path.join(repo, "%s_chm_%s.gnx" % (name, chm)))
    for split in (["train", "val"] if validate else ["train"]):
        cm, _ = model.Confusion_Matrices[split]
        n_digits = int(np.ceil(np.log10(np.max(cm))))
        np.savetxt(os.path.join(repo, "analysis", "confusion_matrix_%s.txt" % split), cm, fmt="%-" + str(n_digits) + ".0f")
        print("Estimated " + split + " accuracy: {}%".format(model.accuracies["smooth_" + split + "_acc"]))
    write_model_config(model, os.path.join(repo, "config.txt"))
    print("Model, info and analysis saved at {}".format(repo))
    if os.environ.get("GNX_CLI_TIMING"):
        sys.stderr.write("gnomix_amd training timings (s): " + ", ".join("%s %.3f" % kv for kv in T.items()) + "\n")
    if base_args["query_file"]:
        print("Launching inference...")
        inf = config.get("inference") or {}
        run_inference(base_args, model, snp_level=bool(inf.get("snp_level_inference")), bed_file_output=bool(inf.get("bed_file_output")),
                      verbose=True, global_ancestry_output=bool(inf.get("global_ancestry_output")),
                      ancestry_allele_freq_output=bool(inf.get("ancestry_allele_freq_output")),
                      ancestry_assoc_output=bool(inf.get("ancestry_assoc_output")), phenotype_file=inf.get("phenotype_file"),
                      ancestry_assoc_model=inf.get("ancestry_assoc_model") or "linear",
                      ancestry_score_output=bool(inf.get("ancestry_score_output")), score_file=inf.get("score_file"),
                      ancestry_mds_output=bool(inf.get("ancestry_mds_output")), ancestry_mds_components=inf.get("ancestry_mds_components"),
                      ancestry_mds_min_sites=inf.get("ancestry_mds_min_sites"),
                      ancestry_clump_output=bool(inf.get("ancestry_clump_output")), ancestry_clump_p1=inf.get("ancestry_clump_p1"),
                      ancestry_clump_p2=inf.get("ancestry_clump_p2"), ancestry_clump_r2=inf.get("ancestry_clump_r2"),
                      ancestry_clump_kb=inf.get("ancestry_clump_kb"), trait_file=inf.get("trait_file"),
                      covariate_file=inf.get("covariate_file"), admixture_mapping_output=bool(inf.get("admixture_mapping_output")),
                      admixture_mapping_perms=inf.get("admixture_mapping_perms"), admixture_mapping_seed=inf.get("admixture_mapping_seed"),
                      admixture_mapping_min_hap=inf.get("admixture_mapping_min_hap"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
