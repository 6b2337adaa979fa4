"""CPU: the numpy rule of pn2_local_pca (tests/normals_ref.py) against the definition, against its mutants, and the shared inputs
against the conditions and caps the GPU test relies on (tests/test_normals_gpu.py makes the same assertions on the kernel)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import normals_ref as NR

CASES = NR.cases()
IDS = [c["name"] for c in CASES]


def test_the_cases_cover_what_they_claim():
    """Wave and workgroup edges, every K, both batch sizes with ragged counts including 0, every pitch."""
    assert {1, 63, 64, 65, 255, 256, 257, 1000} <= {c["N"] for c in CASES}
    assert {1, 2, 3, 4, 7, 8, 9, 16, 31, 32, 33, 64} <= {c["K"] for c in CASES}
    assert {1, 3} <= {c["B"] for c in CASES}
    assert any(c["n_query"] is not None and 0 in c["n_query"].tolist() and c["N"] in c["n_query"].tolist() for c in CASES)
    assert {3, 4, 7} <= {c["ldc"] for c in CASES} and {3, 4, 7} <= {c["ldq"] for c in CASES if c["query"] is not None}
    assert {3, 6, 7} <= {c["ldn"] for c in CASES}
    assert any(c["dist"] is None for c in CASES) and any(c["viewpoint"] is None for c in CASES)
    for c in CASES:                                              # NaN wherever no kernel may read
        assert np.isnan(c["cand"][..., 3:]).all() and (c["query"] is None or np.isnan(c["query"][..., 3:]).all())
    flags = [NR.reference(i)["err"] for i in range(len(CASES))]
    assert {0, NR.ERR_FEW, NR.ERR_NONFINITE} <= set(flags)
    # a slot exactly at the cut-off and one at the next float above, sentinels M and -1, a repeat
    c = CASES[IDS.index("planted")]
    assert (c["dist"] == np.float32(c["max_d2"])).any() and (c["dist"] == np.nextafter(np.float32(c["max_d2"]), np.float32(np.inf))).any()
    assert (c["idx"] == c["M"]).any() and (c["idx"] == -1).any() and (c["idx"][:, ::4, 5] == c["idx"][:, ::4, 4]).all()
    counts = NR.reference(IDS.index("planted"))["count"]
    assert {0, 1, 2} <= set(counts[0, 10:13].tolist())


def _definition(case, ref, b, n):
    """The centred covariance of row (b, n) in exact rational arithmetic on the float32 points, rounded once at the end."""
    c, K, M = case["cand"][b], case["K"], case["M"]
    pts = []
    for k in range(K):
        i = int(case["idx"][b, n, k])
        if 0 <= i < M and not (case["dist"] is not None and case["dist"][b, n, k] > np.float32(case["max_d2"])):
            pts.append([float(x) for x in c[i, :3]])
    cnt = len(pts)
    fm = [sum(Fraction(p[a]) for p in pts) / cnt for a in range(3)]
    C = [float(sum((Fraction(p[a]) - fm[a]) * (Fraction(p[bb]) - fm[bb]) for p in pts) / cnt)
         for a, bb in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return cnt, C


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_rule_against_the_definition(i):
    """cov: the exactly centred covariance (rational arithmetic) to 1e-14 of the neighbourhood's trace on a sample of rows;
    eig / normal: np.linalg.eigh's, through the shared assertions (the reference alone stays inside every bound and cap)."""
    case, ref = CASES[i], NR.reference(i)
    rng = np.random.default_rng(i)
    rows = np.argwhere(ref["written"] & ref["finite"] & (ref["count"] > 0))
    for b, n in rows[rng.permutation(len(rows))[:12]]:
        cnt, C = _definition(case, ref, b, n)
        assert cnt == ref["count"][b, n]
        tr = C[0] + C[3] + C[5]
        assert np.abs(ref["cov"][b, n] - C).max() <= 1e-14 * tr + 1e-300, (case["name"], b, n)
    rec = NR.check_outputs(case, ref, NR.outputs_of(ref, case["ldn"]))
    assert rec["ill"] <= NR.ILL_CAP
    m = ref["written"] & ref["full"]
    if m.any():                                                  # eigh's pair really is one: C u = l0 u, and the trace is kept
        C = NR.full_matrix(ref["cov"][m])
        assert np.abs(ref["l"][m].sum(1) - np.trace(C, axis1=1, axis2=2)).max() <= 1e-14 * max(ref["l"][m][:, 2].max(), 1e-300)


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("mutant", NR.MUTANTS)
def test_every_mutant_fails_on_every_case_it_changes(mutant):
    changed = 0
    for i, case in enumerate(CASES):
        ref = NR.reference(i)
        got = NR.outputs_of(NR.reference(i, mutant), case["ldn"])
        if _same(got, NR.outputs_of(ref, case["ldn"])):
            continue
        changed += 1
        with pytest.raises(AssertionError):
            NR.check_outputs(case, ref, got)
    assert changed >= 3, (mutant, changed)


def test_untouched_columns_and_rows_are_checked():
    i = IDS.index("planted")
    case, ref = CASES[i], NR.reference(i)
    for key, where in (("normal", (0, 0, 5)), ("normal", (1, 200, 0)), ("eig", (2, 64, 1)), ("cov", (1, 100, 0)), ("count", (2, 256))):
        got = NR.outputs_of(ref, case["ldn"])
        got[key][where] = 0
        with pytest.raises(AssertionError):
            NR.check_outputs(case, ref, got)


def test_solver_restatement_converges_within_its_fixed_sweeps():
    """csrc/sym_eig3.h restated (NR.jacobi_eig3): after FOUR sweeps the off-diagonal norm is below 2^-53 of the largest eigenvalue
    on every covariance of the cases and on graded / nearly equal spectra; the kernel runs six.  Its eigenvalues then meet the
    GPU test's bound against eigh, and a diagonal matrix comes back untouched with V = I."""
    rng = np.random.default_rng(0)
    C = np.concatenate([NR.reference(i)["cov"].reshape(-1, 6) for i in range(len(CASES))])
    C = C[np.isfinite(C).all(1)]

    def spectra(R, l):
        Q, _ = np.linalg.qr(rng.standard_normal((R, 3, 3)))
        A = np.einsum("rij,rj,rkj->rik", Q, l, Q)
        return np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], 1)
    near = np.ones((20000, 3))
    near[:, 1] += 1e-13 * rng.random(20000)
    near[:, 2] += 1e-9 * rng.random(20000)
    for M6 in (C, spectra(20000, 10.0 ** (rng.random((20000, 3)) * 30 - 30)), spectra(20000, near)):
        d, V, off = NR.jacobi_eig3(M6, 6)
        l2 = np.abs(d).max(1)
        assert (off[3] <= 2.0 ** -53 * l2).all() and (off[5] <= 2.0 ** -53 * l2).all()
        lam = np.linalg.eigvalsh(NR.full_matrix(M6))
        assert (np.abs(np.sort(d, 1) - lam) <= NR.EIG_ABS_L2 * l2[:, None] + NR.EIG_ABS).all()
        assert np.abs(np.einsum("rji,rjk->rik", V, V) - np.eye(3)).max() <= 2.0 ** -48
    diag = np.zeros((4, 6))
    diag[:, [0, 3, 5]] = [[3, 1, 2], [0, 0, 5], [0, 0, 0], [2, 2, 1]]
    d, V, _ = NR.jacobi_eig3(diag, 6)
    assert (d == diag[:, [0, 3, 5]]).all() and (V == np.eye(3)).all()


HOST_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
#include "sym_eig3.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / 48;
    fseek(f, 0, SEEK_SET);
    std::vector<double> c(n * 6), o(n * 6);
    if (fread(c.data(), 48, n, f) != (size_t)n) return 3;
    fclose(f);
    for (long i = 0; i < n; ++i)
        pn2_sym_eig3(c[6 * i], c[6 * i + 1], c[6 * i + 2], c[6 * i + 3], c[6 * i + 4], c[6 * i + 5], o[6 * i], o[6 * i + 1], o[6 * i + 2],
                     o[6 * i + 3], o[6 * i + 4], o[6 * i + 5]);
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(o.data(), 48, n, g) != (size_t)n) return 4;
    fclose(g);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_kernels_solver_compiled_for_the_host_equals_its_restatement(tmp_path):
    """csrc/sym_eig3.h itself, compiled for the host without contraction (with the address and undefined-behaviour sanitizers where the machine has them), on
    every covariance of the cases: eigenvalues and eigenvector equal NR.jacobi_eig3's bit for bit (sqrt and divide are correctly
    rounded on both sides), the first axis among equal entries included."""
    C = np.concatenate([NR.reference(i)["cov"].reshape(-1, 6) for i in range(len(CASES))])
    C = np.ascontiguousarray(C[np.isfinite(C).all(1)])
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(HOST_MAIN)
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(asan) and os.path.exists(asan) else []
    subprocess.run(["g++", "-O2", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "pointnet12_amd", "csrc"), "-o", str(exe), str(src)], check=True, timeout=300)
    C.tofile(str(tmp_path / "cov.bin"))
    subprocess.run([str(exe), str(tmp_path / "cov.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    o = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 6)
    d, V, _ = NR.jacobi_eig3(C, 6)
    order = np.argsort(d, 1, kind="stable")
    assert np.array_equal(np.take_along_axis(d, order, 1).view(np.uint64), o[:, :3].view(np.uint64))
    assert np.array_equal(V[np.arange(len(C)), :, order[:, 0]].view(np.uint64), o[:, 3:].view(np.uint64))
