#!/usr/bin/env python3
"""Generate tests/golden/g15_chamfer.npz by running the REFERENCE's model/chamfer.py (imported unmodified) on CPU (development
container only, like tools/make_golden_densecls.py).  Per case <c> of ``cases``:

  <c>/p1, <c>/p2       the inputs (float32; the integer-valued ones are exact in it)
  <c>/g                the upstream scalar the gradients were taken for (never 1)
  <c>/value            what the reference returned (float32 run; float64 for ``main*``, which the reference's own __main__ runs so)
  <c>/dp1, <c>/dp2     its autograd gradients
  <c>/argmin           the fp64 arg-min (lowest index on ties), int32
  <c>/fn               "chamfer_batch" or "chamfer_non_batch": the function that was called
  <c>/gap              random cases: the smallest relative gap between the nearest and the next distinct fp64 distance

The reference's own arg-min is observed by wrapping ``torch.min`` while it runs (its text is not touched).  For every random case
this script ASSERTS gap >= 1e-5 and that the reference's fp32 arg-min equals the fp64 one, and moves to the next seed otherwise:
that is what lets tests/test_chamfer_gpu.py demand the arg-min exactly.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_chamfer.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from model import chamfer as R          # noqa: E402  (the reference)
import chamfer_ref as C                 # noqa: E402  (this project's fp64 restatement)

OUT = os.path.join(ROOT, "tests", "golden", "g15_chamfer.npz")
MIN_GAP = 1e-5


class observed_min:
    """While active, ``torch.min(x, dim=...)`` also records the indices it returned."""

    def __enter__(self):
        self.indices = []
        self._orig = torch.min

        def spy(*a, **k):
            r = self._orig(*a, **k)
            if isinstance(r, tuple):
                self.indices.append(r[1].detach().clone())
            return r
        torch.min = spy
        return self

    def __exit__(self, *exc):
        torch.min = self._orig
        return False


def run_reference(fn, p1, p2, g, dtype):
    a = p1.to(dtype).clone().requires_grad_(True)
    b = p2.to(dtype).clone().requires_grad_(True)
    with observed_min() as seen:
        v = getattr(R, fn)(a, b)
    v.backward(torch.tensor(g, dtype=dtype))
    (idx,) = seen.indices
    return v.detach(), a.grad, b.grad, idx.reshape(p1.shape[0], p1.shape[1])


def record(out, name, fn, p1, p2, g, dtype=torch.float32, random=False):
    v, dp1, dp2, ref_idx = run_reference(fn, p1, p2, g, dtype)
    d64, i64 = C.nearest(p1, p2)
    if random:
        gap = C.nearest_gap(p1, p2)
        if gap < MIN_GAP or not bool((ref_idx == i64).all()):
            return False
        out[name + "/gap"] = np.float64(gap)
    out[name + "/p1"], out[name + "/p2"] = p1.numpy(), p2.numpy()
    out[name + "/g"] = np.float64(g)
    out[name + "/value"] = v.numpy()
    out[name + "/dp1"], out[name + "/dp2"] = dp1.numpy(), dp2.numpy()
    out[name + "/argmin"] = i64.numpy().astype(np.int32)
    out[name + "/fn"] = np.array(fn)
    return True


def draw(seed, B, N, M, D):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, D, generator=gen) * 2 - 1, torch.rand(B, M, D, generator=gen) * 2 - 1


def record_random(out, name, fn, B, N, M, D, g, seed, subset=False):
    for s in range(seed, seed + 64):
        p1, p2 = draw(s, B, N, M, D)
        if subset:            # p2: points of p1 picked WITH repeats -> exact zeros, and exact ties at distance 0 between the copies
            pick = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(1000 + s))
            p2 = torch.gather(p1, 1, pick[:, :, None].expand(-1, -1, D)).contiguous()
            assert all(len(set(row.tolist())) < M for row in pick), "no repeat drawn"
        if record(out, name, fn, p1, p2, g, random=True):
            out[name + "/seed"] = np.int64(s)
            return
        print("%s: seed %d refused (gap or fp32 arg-min), trying the next" % (name, s))
    raise SystemExit("%s: no seed passed" % name)


def main():
    out, cases = {}, []

    def add(name):
        cases.append(name)
        return name

    # the two hard-coded point sets of the reference's own __main__ (small integers: exact in float32); it runs them in fp64
    p1 = torch.tensor([[[1., 2, 3], [4, 5, 6], [3, 5, 6], [5, 6, 7]], [[2., 2, 3], [3, 5, 6], [4, 5, 6], [8, 6, 7]]])
    p2 = torch.tensor([[[3., 7, 8], [1, 4, 5]], [[3., 8, 8], [2, 4, 5]]])
    record(out, add("main"), "chamfer_batch", p1, p2, -1.5, torch.float64)
    assert "%.4f" % float(out["main/value"]) == "11.6073", out["main/value"]          # what the reference prints for it
    record(out, add("main_b0"), "chamfer_non_batch", p1[:1], p2[:1], 0.5, torch.float64)
    record(out, add("main_b1"), "chamfer_non_batch", p1[1:], p2[1:], 0.5, torch.float64)
    assert abs((float(out["main_b0/value"]) + float(out["main_b1/value"])) / 2 - float(out["main/value"])) < 1e-12

    record_random(out, add("rand3"), "chamfer_batch", 4, 2048, 1024, 3, 0.75, seed=1)
    for D, N, M in ((2, 301, 203), (4, 333, 190), (6, 257, 129), (9, 195, 321)):
        record_random(out, add("d%d" % D), "chamfer_batch", 3, N, M, D, -2.25, seed=10 * D)
    record_random(out, add("subset"), "chamfer_batch", 2, 500, 300, 3, 1.75, seed=77, subset=True)
    record_random(out, add("nonbatch"), "chamfer_non_batch", 1, 257, 130, 3, 3.0, seed=5)

    # a hand-made three-way tie at NON-zero distance on integer coordinates: query 0 is at distance 1 from candidates 1, 2, 3
    # (candidate 0 is farther), query 1 at sqrt(2) from candidates 1, 2, 3, query 2 coincides with candidates 4 and 5
    t1 = torch.tensor([[[0., 0, 0], [1, 1, 1], [5, 5, 6], [9, 9, 9]]])
    t2 = torch.tensor([[[0., 0, 3], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 6], [5, 5, 6]]])
    record(out, add("tie3"), "chamfer_batch", t1, t2, 2.0)
    assert out["tie3/argmin"].tolist() == [[1, 1, 4, 4]], out["tie3/argmin"]
    assert np.array_equal(out["tie3/dp2"][0, 2:4], np.zeros((2, 3), np.float32))      # the whole gradient went to the lowest index

    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes), cases: %s" % (OUT, os.path.getsize(OUT), " ".join(cases)))
    for c in cases:
        print("  %-9s %-18s p1 %s p2 %s value %.7g%s" % (c, str(out[c + "/fn"]), out[c + "/p1"].shape, out[c + "/p2"].shape,
                                                         float(out[c + "/value"]), "  gap %.2e" % out[c + "/gap"] if c + "/gap" in out else ""))


if __name__ == "__main__":
    main()
