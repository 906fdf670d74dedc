"""gnx_exp.h's exp (the CRF potentials, Gnofix's softmax exponentials) and the logistic kernels' reciprocal and sigmoid (gnx_rcp_nr,
gnx_sigmoidN) restated on the host with THE HEADER'S OWN constants.

The device function is a fixed sequence of IEEE operations (v_mul_f64, v_rndne_f64, v_fma_f64, v_cvt_i32_f64, v_ldexp_f64), so the
same sequence in C with fma() / rint() / ldexp() yields the same bits for every argument; what can go wrong is a constant.  The
constants are parsed out of gnomix_amd/csrc/gnx_exp.h (in the order the function uses them), compiled into a small C program and
compared with glibc's exp over 3e6 arguments in [-745, 709]: within 2 units of the last place, exact behaviour at the ends.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SRC = r"""
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
static double K(uint32_t lo, uint32_t hi) { uint64_t b = ((uint64_t)hi << 32) | lo; double d; memcpy(&d, &b, 8); return d; }
static const uint32_t C[][2] = { %s };
static double exp_sc(double x) {
  double n = rint(x * K(C[0][0], C[0][1]));
  double r = fma(n, K(C[1][0], C[1][1]), x);
  r = fma(n, K(C[2][0], C[2][1]), r);
  double p = K(C[3][0], C[3][1]);
  for (int i = 4; i < %d; ++i) p = fma(p, r, K(C[i][0], C[i][1]));
  p = fma(p, r, 0.5); p = fma(p, r, 1.0); p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}
int main(void) {
  double worst = 0.0; uint64_t s = 88172645463325252ULL; long bad = 0;
  for (long i = 0; i < 3000000; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const double u = (double)(s >> 11) / 9007199254740992.0;
    const double x = (i %% 3 == 0) ? -745.0 + u * 1454.0 : (i %% 3 == 1 ? -40.0 + u * 80.0 : -1.0 + u * 2.0);
    const double a = exp_sc(x), b = exp(x);
    if (b > 1e-300 && b < 1e300) { const double e = fabs(a - b) / b; if (e > worst) worst = e; if (e > 4.5e-16) ++bad; }
  }
  printf("%%.3e %%ld %%g %%g %%g %%.17g\n", worst, bad, exp_sc(0.0), exp_sc(710.0), exp_sc(-800.0), exp_sc(1.0));
  return 0;
}
"""


def test_exp_sc_constants_and_accuracy(tmp_path):
    hdr = open(os.path.join(ROOT, "gnomix_amd", "csrc", "gnx_exp.h")).read()
    body = hdr[hdr.index("void gnx_exp_scN(double (&x)[N])"):hdr.index("__device__ __forceinline__ double gnx_exp_sc(double x)")]
    consts = re.findall(r"<0x([0-9a-fA-F]{8})u, 0x([0-9a-fA-F]{8})u", body)
    # in the order the function uses them: 1/ln2, -ln2_hi, -ln2_lo, 1/13!, 1/12!, .., 1/3!
    assert len(consts) == 14
    order = consts
    table = ", ".join("{0x%su, 0x%su}" % c for c in order)
    src = tmp_path / "exp_sc.c"
    src.write_text(C_SRC % (table, len(order)))
    exe = tmp_path / "exp_sc"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    worst, bad = float(out[0]), int(out[1])
    assert worst < 4.5e-16 and bad == 0, out          # 2 units of the last place of the value
    assert float(out[2]) == 1.0 and out[3] == "inf" and float(out[4]) == 0.0
    import math
    assert abs(float(out[5]) - math.e) < 1e-15


# gnx_rcp_nr / gnx_sigmoidN: v_rcp_f64 seeds two Newton steps made of fma.  The hardware seed is not reproducible on the host (the ISA
# promises about float32 precision), so the restatement takes the seed as a parameter: the exact reciprocal, the reciprocal rounded to a
# float32's 24 bits, and both perturbed by +-2^-20 relative — far coarser than the instruction.  What is checked: every seed ends
# within 1 ulp of 1 / y (the header's claim), the seeds' results are within 1 ulp of each other (so the device's cannot differ by more),
# and 1 / (1 + e^-t) is within exp's 4.5e-16 + 2^-53 (the addition) + 2^-52 (the reciprocal) of the long double value over [-745, 745].
C_SIG = r"""
static double seed(double y, int mode) {
  double r = 1.0 / y;
  if (mode & 1) { int e; double m = frexp(r, &e); r = ldexp((double)(float)m, e); }
  if (mode & 2) r *= 1.0 + 0x1p-20;
  if (mode & 4) r *= 1.0 - 0x1p-20;
  return r;
}
static double rcp_nr(double y, int mode) {
  double r = seed(y, mode);
  double e = fma(-y, r, 1.0);
  r = fma(r, e, r);
  e = fma(-y, r, 1.0);
  return fma(r, e, r);
}
static double sigmoid(double t, int mode) { return rcp_nr(1.0 + exp_sc(fmax(fmin(-t, 708.0), -746.0)), mode); }
static double ulps(double a, double b) { int e; frexp(b, &e); return fabs(a - b) / ldexp(1.0, e - 53); }
int main2(void) {
  uint64_t s = 88172645463325252ULL;
  double w_rcp = 0.0, w_seed = 0.0, w_sig = 0.0;
  const int modes[6] = {0, 1, 2, 4, 3, 5};
  for (long i = 0; i < 1000000; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const double u = (double)(s >> 11) / 9007199254740992.0;
    const double t = (i %% 3 == 0) ? -745.0 + u * 1490.0 : (i %% 3 == 1 ? -40.0 + u * 80.0 : -709.0 + u * 2.0);
    const double y = 1.0 + exp_sc(fmin(-t, 708.0));
    const long double exact = 1.0L / (long double)y;
    const double r0 = rcp_nr(y, 0);
    for (int k = 0; k < 6; ++k) {
      const double r = rcp_nr(y, modes[k]);
      const double e = (double)(fabsl((long double)r - exact) / exact);
      if (e > w_rcp) w_rcp = e;
      if (ulps(r, r0) > w_seed) w_seed = ulps(r, r0);
    }
    if (-t <= 708.0) {
      const long double want = 1.0L / (1.0L + expl(-(long double)t));
      const double e = (double)(fabsl((long double)sigmoid(t, 1) - want) / want);
      if (e > w_sig) w_sig = e;
    }
  }
  printf("%%.3e %%.3f %%.3e %%.17g %%.17g %%d %%d\n", w_rcp, w_seed, w_sig, sigmoid(1e300, 1), sigmoid(-1e300, 1),
         sigmoid(-1e300, 1) == sigmoid(-708.0, 1), sigmoid(-709.9, 0) == sigmoid(-708.0, 5));
  return 0;
}
"""


def test_rcp_and_sigmoid_newton_steps(tmp_path):
    hdr = open(os.path.join(ROOT, "gnomix_amd", "csrc", "gnx_exp.h")).read()
    body = hdr[hdr.index("void gnx_exp_scN(double (&x)[N])"):hdr.index("__device__ __forceinline__ double gnx_exp_sc(double x)")]
    consts = re.findall(r"<0x([0-9a-fA-F]{8})u, 0x([0-9a-fA-F]{8})u", body)
    assert len(consts) == 14
    # the header's own Newton sequence and cap, so that the restatement above is the header's: two steps of (fma(-y, r, 1), fma(r, e, r))
    sig = hdr[hdr.index("__device__ __forceinline__ double gnx_rcp_nr(double y)"):hdr.index("#else   // host pass")]
    assert sig.count("__builtin_fma(-y, r, 1.0)") == 2 and sig.count("__builtin_fma(r, e, r)") == 2
    assert "__builtin_fmax(__builtin_fmin(-v[i], 708.0), -746.0)" in sig and sig.count("__builtin_fma(-v[i], r[i], 1.0)") == 2 and sig.count("__builtin_fma(r[i], e[i], r[i])") == 2
    table = ", ".join("{0x%su, 0x%su}" % c for c in consts)
    main1 = C_SRC[C_SRC.index("int main(void)"):]
    src = tmp_path / "sig.c"
    src.write_text((C_SRC.replace(main1, "") + C_SIG + "int main(void) { return main2(); }\n") % (table, len(consts)))
    exe = tmp_path / "sig"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    print(out)
    assert float(out[0]) <= 2.0 ** -52, out            # gnx_rcp_nr: within 1 ulp of 1 / y from every seed
    assert float(out[1]) <= 1.0, out                   # seeds 2^-20 apart end within 1 ulp of each other
    assert float(out[2]) <= 4.5e-16 + 2.0 ** -53 + 2.0 ** -52, out
    assert float(out[3]) == 1.0 and 0.0 < float(out[4]) < 4e-308 and out[5] == "1" and out[6] == "1"   # saturated ends: 1, and the cap's 3.3e-308
