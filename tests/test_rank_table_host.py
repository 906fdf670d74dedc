"""The rank table of the tree smoother (gnomix_amd/csrc/gnx_rank_table.h) on the host, no GPU.

The header is plain C++: the builder the model loader runs and the pieces of the lookup the kernels run (bucket, entry, bisection).
A small stand-alone program includes it, builds the table of a threshold set — by the sizing rule and at the forced sizes 2^4, 2^10,
2^12, 2^14, 2^16 — and compares gnx_rank_lookup with brute force, r(p) = #{k : U[k] <= p} (NaN -> 0xFFFF), at every bucket
boundary, every threshold, the two float neighbours of each, and the special values.  An off-by-one in the table shows here first."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CPP_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gnx_rank_table.h"

static uint32_t brute(const std::vector<float>& U, float p) {
  if (p != p) return 0xFFFFu;
  uint32_t r = 0;
  for (float u : U) r += (u <= p) ? 1u : 0u;
  return r;
}

int main(int argc, char** argv) {
  std::vector<float> U;
  FILE* f = std::fopen(argv[1], "rb");
  float v;
  while (std::fread(&v, 4, 1, f) == 1) U.push_back(v);
  std::fclose(f);
  const float inf = std::numeric_limits<float>::infinity();
  for (int a = 2; a < argc; ++a) {
    const int force = std::atoi(argv[a]);
    GnxRankTable T;
    gnx_rank_table_build(U, force, T);
    const int NB = 1 << T.bits;
    std::vector<float> probe = {0.0f, 1.0f, -0.0f, 1.5f, -1.0f, std::numeric_limits<float>::quiet_NaN(), inf, -inf,
                                std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), 1e-40f,
                                std::numeric_limits<float>::min(), std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), 3e38f};
    auto with_neighbours = [&](float x) {
      probe.push_back(x);
      probe.push_back(std::nextafter(x, -inf));
      probe.push_back(std::nextafter(x, inf));
    };
    for (int b = 0; b <= NB; ++b) with_neighbours((float)b / (float)NB);
    for (float u : U) with_neighbours(u);
    // brute force by a sorted sweep would hide nothing, but K x probes is too slow for the large sets: count with upper_bound, and
    // check upper_bound itself against the plain loop on a sample
    long bad = 0, n = 0;
    for (size_t i = 0; i < probe.size(); ++i) {
      const float p = probe[i];
      uint32_t want = (p != p) ? 0xFFFFu : (uint32_t)(std::upper_bound(U.begin(), U.end(), p) - U.begin());
      if (i % 97 == 0 || i < 64) { if (want != brute(U, p)) { ++bad; } }
      const uint32_t got = gnx_rank_lookup(U, T, p);
      if (got != want) { if (bad < 5) std::fprintf(stderr, "bits %d p %.9g: got %u want %u\n", T.bits, (double)p, got, want); ++bad; }
      ++n;
    }
    // the entry layout itself
    long bad_entry = 0;
    for (int b = 0; b < NB; ++b) {
      const GnxRankEntry& e = T.lut[(size_t)b];
      const int lo = (int)(e.lohi & 0xffffu), hi = (int)(e.lohi >> 16);
      if (lo > hi || hi > (int)U.size() || hi - lo > T.fullest) ++bad_entry;
      for (int i = 0; i < GNX_RANK_INLINE; ++i) {
        if (i < hi - lo) { if (std::memcmp(&e.t[i], &U[(size_t)(lo + i)], 4) != 0) ++bad_entry; }
        else if (e.t[i] == e.t[i]) ++bad_entry;
      }
      if (b > 0 && (int)(T.lut[(size_t)(b - 1)].lohi >> 16) != lo) ++bad_entry;
    }
    if ((T.lut[0].lohi & 0xffffu) != 0 || (int)(T.lut[(size_t)NB - 1].lohi >> 16) != (int)U.size()) ++bad_entry;
    std::printf("%d %d %d %d %ld %ld %ld\n", force, T.bits, T.steps, T.fullest, n, bad, bad_entry);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rank_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_table")
    src = d / "rank_table_host.cpp"
    src.write_text(CPP_SRC)
    exe = d / "rank_table_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "gnomix_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)
    return exe, d


def threshold_sets():
    """name -> sorted distinct float32 thresholds (what build_xgb_rk hands the builder); shared with tests/test_gpu_rank_table.py"""
    from gnomix_amd import synth
    rng = np.random.RandomState(7)
    bench = synth.synthetic_model(seed=0, n_rounds=100, **synth.CHR22)
    sets = {
        "bench_uniform": bench.cond[bench.left != -1],
        "one_1024th": (307.0 / 1024.0 + rng.random_sample(2000) / 1024.0 * 0.999).astype(np.float32),   # all inside [307/1024, 308/1024)
        "single": np.array([0.37], np.float32),
        "edges": np.array([0.0, 1.0, np.finfo(np.float32).smallest_subnormal], np.float32),
        "large": rng.random_sample(40000).astype(np.float32),
        "outside": np.array([-3.0, -1e-30, 0.25, 0.25 + 2.0 ** -20, 0.25 + 2.0 ** -19, 0.25 + 2.0 ** -18, 0.25 + 2.0 ** -17, 2.0, 1e30], np.float32),
    }
    return {k: np.unique(v[np.isfinite(v)].astype(np.float32)) for k, v in sets.items()}


@pytest.mark.parametrize("name", ["bench_uniform", "one_1024th", "single", "edges", "large", "outside"])
def test_rank_table_against_brute_force(rank_exe, name):
    exe, d = rank_exe
    U = threshold_sets()[name]
    path = d / (name + ".f32")
    U.tofile(str(path))
    out = subprocess.run([str(exe), str(path), "0", "4", "10", "12", "14", "16"], check=True, capture_output=True, text=True)
    rows = [[int(x) for x in ln.split()] for ln in out.stdout.strip().split("\n")]
    assert len(rows) == 6, out.stderr
    for force, bits, steps, fullest, n, bad, bad_entry in rows:
        assert bad == 0 and bad_entry == 0, (name, force, out.stderr)
        assert n >= 3 * ((1 << bits) + len(U))
        assert bits == (force if force else bits)
        # steps: the smallest count that resolves what the fullest bucket keeps behind its entry
        rest = fullest - 3
        assert steps == (0 if rest <= 0 else int(np.ceil(np.log2(rest + 1))))
    rule = rows[0]
    # the rule: the smallest table from 2^10 up whose buckets all fit their entry, else the largest
    assert 10 <= rule[1] <= 16 and (rule[2] == 0 or rule[1] == 16)
    if rule[1] > 10:
        smaller = subprocess.run([str(exe), str(path), str(rule[1] - 1)], check=True, capture_output=True, text=True).stdout.split()
        assert int(smaller[2]) > 0
    if name == "one_1024th":
        assert rows[2][2] > 1 and rule[2] > 1     # the fullest-bucket path: more than one bisection at 2^10 and under the rule
    if name in ("single", "edges"):
        assert rule[1] == 10 and rule[2] == 0
    if name == "large":
        assert rule[1] == 16
