"""CPU: the launch geometry of k_step_multi (gym_auv_amd/csrc/auv_multi_geom.h), compiled with the host compiler.

The header is the one source of the kernel's workgroup decode, the launcher's grid and auv_step_multi's checks.  These tests
check that every workgroup of a launch decodes to a distinct (step, role, index) and every one of those is dispatched exactly
once, in an order where each producer is ahead of its consumer; that the cohort order's division by the cohort count is exact
at every size the host accepts (the multiplier ceil(2^32 / C) alone is one too high from some q on, unless C is a power of
two); and that the host's verdict on the dispatch limit (2^32 - 1 work-items) is the exact product's."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_auv_amd", "csrc")
CXX = shutil.which("g++")
LIMIT = (1 << 32) - 1

SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "auv_multi_geom.h"

static long long n_checked = 0;

// every workgroup of the launch decodes inside its role's count or to "outside"; every (step, role, bi) exactly once; in
// dispatch position: dynamics(e, s) < sweep(e, s), search(e, s) < finish(e, s) < dynamics(e, s + 1)
static int check_decode(int ne, int n_steps, int order, int lead, int lag) {
  const AuvMultiGeom g = auv_multi_geom(ne, n_steps, order, lead, lag);
  if ((g.lead >= 0) != (order == 1 && ne % 64 == 0 && ne / 64 >= 3)) { printf("order ne=%d order=%d lead=%d\n", ne, order, g.lead); return 1; }
  const int nk = auv_multi_dyn_waves(ne), cnt[4] = {nk, ne, ne, nk};
  std::vector<long long> pos[4];
  for (int r = 0; r < 4; r++) pos[r].assign((size_t)n_steps * cnt[r], -1);
  const unsigned long long grid = auv_multi_grid(g);
  for (unsigned long long b = 0; b < grid; b++) {
    const unsigned bx = (unsigned)b;
    const AuvMultiWave w = g.lead >= 0 ? auv_multi_decode_cohorts(bx, ne, n_steps, g.lead, g.lag, g.magic) : auv_multi_decode_steps(bx, ne, n_steps);
    n_checked++;
    if (w.step == n_steps) continue;
    if (w.step < 0 || w.step > n_steps || w.role < 0 || w.role > 3 || w.bi < 0 || w.bi >= cnt[w.role]) {
      printf("range ne=%d n=%d order=%d lead=%d lag=%d bx=%u -> step %d role %d bi %d\n", ne, n_steps, order, g.lead, g.lag, bx, w.step, w.role, w.bi);
      return 1;
    }
    long long& slot = pos[w.role][(size_t)w.step * cnt[w.role] + w.bi];
    if (slot >= 0) {
      printf("twice ne=%d n=%d order=%d lead=%d lag=%d bx=%u and %lld -> step %d role %d bi %d\n", ne, n_steps, order, g.lead, g.lag, bx, slot, w.step, w.role, w.bi);
      return 1;
    }
    slot = (long long)bx;
  }
  for (int r = 0; r < 4; r++)
    for (size_t i = 0; i < pos[r].size(); i++)
      if (pos[r][i] < 0) { printf("missing ne=%d n=%d order=%d role %d step %zu bi %zu\n", ne, n_steps, order, r, i / cnt[r], i % cnt[r]); return 1; }
  for (int s = 0; s < n_steps; s++)
    for (int e = 0; e < ne; e++) {
      const int wv = 8 * (e / 64) + e % 8;                 // the dynamics / finish wave of environment e
      const long long D = pos[0][(size_t)s * nk + wv], S = pos[1][(size_t)s * ne + e], N = pos[2][(size_t)s * ne + e], F = pos[3][(size_t)s * nk + wv];
      const long long D1 = s + 1 < n_steps ? pos[0][(size_t)(s + 1) * nk + wv] : 0x7fffffffffffll;
      if (!(D < S && D < N && S < F && N < F && F < D1)) {
        printf("order ne=%d n=%d order=%d lead=%d lag=%d step %d env %d: dyn %lld sweep %lld search %lld finish %lld next dyn %lld\n", ne, n_steps,
               order, g.lead, g.lag, s, e, D, S, N, F, D1);
        return 1;
      }
    }
  return 0;
}

// the decode at the dynamics and finish positions of every q < n_steps * C (ne = 64 C) against q / C, q % C
static int check_exact_decode(int C, int n_steps) {
  const AuvMultiGeom g = auv_multi_geom(64 * C, n_steps, 1, 16, 30);
  for (long long q = 0; q < (long long)n_steps * C; q++) {
    const int s = (int)(q / C), c = (int)(q % C), k = (int)(q % 8);
    const AuvMultiWave a = auv_multi_decode_cohorts((unsigned)(144 * q + k), 64 * C, n_steps, g.lead, g.lag, g.magic);
    const AuvMultiWave f = auv_multi_decode_cohorts((unsigned)(144 * (q + g.lead + g.lag) + 136 + k), 64 * C, n_steps, g.lead, g.lag, g.magic);
    n_checked += 2;
    if (a.step != s || a.role != 0 || a.bi != 8 * c + k || f.step != s || f.role != 3 || f.bi != 8 * c + k) {
      printf("inexact C=%d q=%lld: dynamics (%d, %d, %d), finish (%d, %d, %d), want step %d bi %d\n", C, q, a.step, a.role, a.bi, f.step, f.role, f.bi, s, 8 * c + k);
      return 1;
    }
  }
  return 0;
}

// For a fixed step s, the estimate floor(q * m / 2^32) is nondecreasing in q and never below s on [s C, s C + C): it is too high
// on a tail of that range, and highest at its last position q = s C + C - 1.  If the division is exact there (the estimate at
// most s + 1, and corrected), every q of the range has estimate s or s + 1 and is exact too.  So q = s C + C - 1, s < 1024,
// covers every q < 1024 C.  (q = s C is checked as well: the smallest estimate of the range.)
static int check_exact_div(int c0, int c1) {
  for (int C = c0; C <= c1; C++) {
    const unsigned m = auv_multi_magic(C);
    for (int s = 0; s < 1024; s++)
      for (int k = 0; k < 2; k++) {
        const unsigned q = (unsigned)s * (unsigned)C + (k ? (unsigned)C - 1u : 0u);
        int r;
        const int t = auv_multi_div(q, C, m, &r);
        n_checked++;
        if (t != s || r != (k ? C - 1 : 0)) { printf("inexact C=%d q=%u: %d rem %d\n", C, q, t, r); return 1; }
      }
  }
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argv[1];
  if (!strcmp(mode, "decode")) {
    // lines: ne n_steps order lead lag
    int ne, n, o, lead, lag;
    while (scanf("%d %d %d %d %d", &ne, &n, &o, &lead, &lag) == 5)
      if (check_decode(ne, n, o, lead, lag)) return 1;
  } else if (!strcmp(mode, "exact")) {
    const int cs[] = {2731, 4095, 4097, 5461, 8191, 8193, 10923, 16383};
    for (int C : cs)
      if (check_exact_decode(C, 1024)) return 1;
    if (check_exact_div(3, 32768)) return 1;
  } else if (!strcmp(mode, "limit")) {
    // lines: ne n_steps order lead lag -> grid lead lag fits
    int ne, n, o, lead, lag;
    while (scanf("%d %d %d %d %d", &ne, &n, &o, &lead, &lag) == 5) {
      const AuvMultiGeom g = auv_multi_geom(ne, n, o, lead, lag);
      printf("%llu %d %d %d\n", auv_multi_grid(g), g.lead, g.lag, (int)auv_multi_fits(g));
    }
    return 0;
  }
  printf("ok %lld\n", n_checked);
  return 0;
}
"""


@pytest.fixture(scope="module")
def geom_bin():
    if CXX is None:
        pytest.skip("g++ not installed")
    tmp = tempfile.mkdtemp(prefix="auv_geom_")
    open(os.path.join(tmp, "t.cpp"), "w").write(SRC)
    subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", "t", "t.cpp"], cwd=tmp, check=True)
    yield os.path.join(tmp, "t")
    shutil.rmtree(tmp, ignore_errors=True)


def _run(exe, mode, lines=()):
    out = subprocess.run([exe, mode], input="".join("%d %d %d %d %d\n" % tuple(l) for l in lines), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _clamp(C, lead, lag):
    """The rule, as the documentation states it: lead, lag >= 1; lead + lag <= C - 1, cut from the larger first."""
    lead, lag = max(lead, 1), max(lag, 1)
    while lead + lag > C - 1:
        if lag > lead and lag > 1:
            lag -= 1
        elif lead > 1:
            lead -= 1
        else:
            lag -= 1
    return lead, lag


LEAD_LAG = [(16, 30), (0, 0), (1, 1), (4096, 4096), (1, 30), (30, 1)]


def test_decode_covers_every_wave_once_in_producer_order(geom_bin):
    cases = []
    for C in range(1, 71):
        for ne in (64 * C - 1, 64 * C, 64 * C + 1):
            steps = (1, 2, 3, 7, 64) + ((1024,) if C <= 6 else ())
            for n in steps:
                cases.append((ne, n, 0, 16, 30))
                if ne % 64 == 0 and C >= 3:
                    cases += [(ne, n, 1, lead, lag) for lead, lag in LEAD_LAG]
                else:
                    cases.append((ne, n, 1, 16, 30))              # (falls back to step-major)
    # the GPU test's slice past the old bound: C = 10923, the multiplier alone is wrong from step 36 on
    cases += [(699072, 40, 1, 16, 30), (699072, 40, 0, 16, 30)]
    out = _run(geom_bin, "decode", cases)
    assert out.startswith("ok"), out


def test_cohort_division_is_exact(geom_bin):
    out = _run(geom_bin, "exact")
    assert out.startswith("ok"), out


def test_clamp_keeps_producers_ahead_and_requests_that_fit(geom_bin):
    lines = [(64 * C, 1, 1, lead, lag) for C in range(3, 200) for lead, lag in LEAD_LAG + [(2, 60), (60, 2), (100, 100)]]
    rows = [tuple(map(int, l.split())) for l in _run(geom_bin, "limit", lines).split("\n") if l]
    for (ne, _, _, lead, lag), (_, gl, gg, _) in zip(lines, rows):
        C = ne // 64
        assert (gl, gg) == _clamp(C, lead, lag), (C, lead, lag, gl, gg)
        assert gl >= 1 and gg >= 1 and gl + gg <= C - 1
        if 1 <= lead and 1 <= lag and lead + lag <= C - 1:
            assert (gl, gg) == (lead, lag)


def _items(ne, n, order, lead, lag):
    """The exact work-item count of the launch, in Python integers."""
    if order == 1 and ne % 64 == 0 and ne // 64 >= 3:
        lead, lag = _clamp(ne // 64, lead, lag)
        return (n * (ne // 64) + lead + lag) * 144 * 64
    return n * (2 * 8 * -(-ne // 64) + 2 * 8 * -(-ne // 8)) * 64


def test_dispatch_limit_verdict_is_the_exact_products(geom_bin):
    lines = []
    for n in (1, 2, 7, 28, 40, 64, 300, 1024):
        for order, (lead, lag) in [(0, (16, 30)), (1, (16, 30)), (1, (0, 0)), (1, (4096, 4096))]:
            # the smallest ne whose launch no longer fits (the count is nondecreasing in ne), and every ne within 200 of it
            lo, hi = 1, 1 << 30
            while lo < hi:
                mid = (lo + hi) // 2
                if _items(mid, n, order, lead, lag) > LIMIT:
                    hi = mid
                else:
                    lo = mid + 1
            lines += [(ne, n, order, lead, lag) for ne in range(max(1, lo - 200), lo + 200)]
    # the issue's examples: 32768 envs x 1024 steps (75.5 M workgroups: within 0x7fffffff, past 2^32 work-items), the GPU test's
    # slice past the old bound
    lines += [(32768, 1024, 0, 16, 30), (32768, 1024, 1, 16, 30), (699072, 40, 1, 16, 30), (699072, 40, 0, 16, 30), (699072, 43, 1, 16, 30)]
    rows = [tuple(map(int, l.split())) for l in _run(geom_bin, "limit", lines).split("\n") if l]
    assert len(rows) == len(lines)
    fits = {}
    for l, (grid, _, _, ok) in zip(lines, rows):
        items = _items(*l)
        assert grid * 64 == items, (l, grid)
        assert ok == (items <= LIMIT), (l, items, ok)
        fits[l] = ok
    assert sum(fits.values()) and not all(fits.values())
    assert not fits[(32768, 1024, 0, 16, 30)] and not fits[(32768, 1024, 1, 16, 30)]
    assert fits[(699072, 40, 1, 16, 30)] and fits[(699072, 40, 0, 16, 30)] and not fits[(699072, 43, 1, 16, 30)]
