"""Weights for the ancestry-partitioned polygenic scores of gnx_ancestry_score (include/gnomix_hip.h): from an
association result of this package, or from a score file.  The scoring itself is the device's (DeviceModel.ancestry_scores[_device /
_gt2], HipGnomix.ancestry_scores); the .sscore.tsv writer is postprocess.write_sscore."""
import math

import numpy as np

EFFECT_REF, EFFECT_ALT, EFFECT_NONE = 0, 1, 255    # the bytes of gnx_ancestry_score's effect array


def weights_from_assoc(res, p_max=None, index_of=None):
    """(C, A) float64 weights from an assoc.AncestryAssoc or assoc.AncestryAssocLogit: its beta (per ALT allele on a haplotype of that
    ancestry, so the effect allele is ALT everywhere), 0 where beta is NaN (a dropped term, a SNP that was not fitted) or not finite;
    with p_max also 0 where p > p_max or p is NaN; with index_of ((C, A) int64, HipGnomix.ancestry_clump's: column a from ld.clump) also 0
    wherever the SNP is not its own index SNP in that ancestry, so that of every clump only the strongest SNP is scored"""
    beta = np.array(res.beta, dtype=np.float64)
    keep = np.isfinite(beta)
    if p_max is not None:
        p = np.asarray(res.p, dtype=np.float64)
        keep &= np.isfinite(p) & (p <= float(p_max))
    if index_of is not None:
        idx = np.asarray(index_of)
        if idx.shape != beta.shape:
            raise ValueError(f"index_of must be {beta.shape} as beta is, got {idx.shape}")
        keep &= idx == np.arange(beta.shape[0])[:, None]
    return np.where(keep, beta, 0.0)


def read_score_file(path, chm, snp_pos, snp_ref, snp_alt, population_order):
    """a score file for the model's SNPs -> (weights (C, A, S) float64, effect (C,) uint8, names [S], report).

    The file is a TSV.  Its header is `chm  pos  effect_allele` followed by one or more weight columns.  A weight column is named NAME
    (one weight for every ancestry) or NAME:POP (the weight of population POP of `population_order` only; a population without a
    column gets 0 for that score).  A NAME given both ways, a NAME:POP given twice or an unknown POP is an error.  Scores come in the
    order of their first column.  Rows of another chromosome are ignored.  A position the model lacks, or an effect allele that is
    neither the model's REF nor its ALT there, is left out and counted in report["not_in_model"] / report["allele_mismatch"]; a (chm,
    pos) listed twice, a cell that is empty, NA or not a finite number, or a line with another number of cells is an error.
    effect[c] is 1 where the effect allele is the model's ALT, 0 where it is its REF and 255 at model SNPs the file does not score
    (report["scored"] of them are scored, report["other_chm"] rows were ignored)."""
    pos = np.asarray(snp_pos).astype(np.int64)
    ref, alt = [str(x) for x in np.asarray(snp_ref)], [str(x) for x in np.asarray(snp_alt)]
    pops = [str(p) for p in population_order]
    C, A = len(pos), len(pops)
    with open(path) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f if ln.strip()]
    if not lines:
        raise ValueError(f"{path}: empty score file")
    head = lines[0].split("\t")
    if len(head) < 4 or head[:3] != ["chm", "pos", "effect_allele"]:
        raise ValueError(f"{path}: the header must be 'chm<TAB>pos<TAB>effect_allele' and at least one weight column, got {head[:4]}")
    names, plain, targets = [], set(), []      # targets[j] = (score index, population index or None) of weight column j
    seen = set()
    for col in head[3:]:
        name, sep, pop = col.partition(":")
        if not name:
            raise ValueError(f"{path}: a weight column has no name: '{col}'")
        if sep and pop not in pops:
            raise ValueError(f"{path}: column '{col}' names a population the model lacks (it has {pops})")
        if col in seen:
            raise ValueError(f"{path}: column '{col}' is given twice")
        seen.add(col)
        if name not in names:
            names.append(name)
            if not sep:
                plain.add(name)
        elif (name in plain) != (not sep) or not sep:
            raise ValueError(f"{path}: score '{name}' is given both as '{name}' and as '{name}:POP'")
        targets.append((names.index(name), pops.index(pop) if sep else None))
    S = len(names)
    where = {int(p): c for c, p in enumerate(pos)}
    weights = np.zeros((C, A, S))
    effect = np.full(C, EFFECT_NONE, np.uint8)
    report = {"scored": 0, "other_chm": 0, "not_in_model": 0, "allele_mismatch": 0}
    listed = set()
    for ln in lines[1:]:
        cells = ln.split("\t")
        if len(cells) != len(head):
            raise ValueError(f"{path}: a line has {len(cells)} cells, the header {len(head)}")
        if cells[0].strip() != str(chm):
            report["other_chm"] += 1
            continue
        try:
            p = int(cells[1].strip())
        except ValueError:
            raise ValueError(f"{path}: '{cells[1]}' is not a position") from None
        if p in listed:
            raise ValueError(f"{path}: chromosome {chm} position {p} is listed twice")
        listed.add(p)
        vals = []
        for cell in cells[3:]:
            cell = cell.strip()
            try:
                v = float(cell) if cell and cell.upper() != "NA" else math.nan
            except ValueError:
                v = math.nan
            if not math.isfinite(v):
                raise ValueError(f"{path}: chromosome {chm} position {p}: weight '{cell}' is not a finite number")
            vals.append(v)
        c = where.get(p)
        if c is None:
            report["not_in_model"] += 1
            continue
        allele = cells[2].strip()
        if allele == alt[c]:
            effect[c] = EFFECT_ALT
        elif allele == ref[c]:
            effect[c] = EFFECT_REF
        else:
            report["allele_mismatch"] += 1
            continue
        report["scored"] += 1
        for (s, a), v in zip(targets, vals):
            if a is None:
                weights[c, :, s] = v
            else:
                weights[c, a, s] = v
    return weights, effect, names, report
