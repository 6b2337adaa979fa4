"""What the conv1x1 backward entry points answer to a bad upstream-gradient operand (no GPU needed, nothing is launched).

"This layer's output gradient" reaches seven entry points of include/pn2.h as the same nine arguments -- dense (dZ, ldz) or
implied by the max-pool (dZp, ldo, arg, Kpool), with Y, ldy, coef and an optional lazy coefficient record.  Which code a call
returns when the operand is wrong, and which check wins when two are violated, is part of the ABI: the table below records it.
Every case fails a host-side check in front of the first device call of its entry point (read off csrc/mlp.hip and
csrc/mlp_res.hip: pn2_conv1x1_dgrad and pn2_conv1x1_bwd_pair look up a device symbol before they check the pitch of dZ / dZp, so
the ldz / ldo cases are left out for those two).  Pointers are dummy integers that are never dereferenced."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED = -1, -3
FAKE = 1 << 20                  # 256-byte aligned, never dereferenced
ROWS = 1 << 20

# argument names in the order of include/pn2.h
ORDER = {
    "pn2_conv1x1_dgrad": "dZ ldz dZp ldo arg Kpool Y ldy coef W ldw prev_Y ld_prev prev_affine dXout ldxo prev_red P C_out C_in "
                         "coef_lazy stream",
    "pn2_conv1x1_wgrad": "dZ ldz dZp ldo arg Kpool Y ldy coef X ldx x_affine dW lddw dbias P C_out C_in coef_lazy stream",
    "pn2_conv1x1_wgrad_ws": "dZ ldz dZp ldo arg Kpool Y ldy coef X ldx x_affine dW lddw dbias P C_out C_in coef_lazy workspace stream",
    "pn2_conv1x1_bwd_pair": "dZ ldz dZp ldo arg Kpool Y ldy coef W ldw prev_Y ld_prev prev_affine dXout ldxo prev_red X ldx x_affine "
                            "dW lddw P C_out C_in coef_lazy stream",
    "pn2_conv1x1_bwd": "dZ ldz dZp ldo arg Kpool Y ldy coef W ldw prev_Y ld_prev prev_affine dXout ldxo prev_red dW lddw P C_out C_in "
                       "coef_lazy stream",
    "pn2_conv1x1_bwd_cf": "dZp ldo arg Kpool coef W ldw bias prev_Y ld_prev prev_affine dXout ldxo prev_red dW lddw P C_out C_in "
                          "coef_lazy scratch stream",
    "pn2_conv1x1_bwd_first": "dZ ldz Y ldy coef W ldw prev_Y ld_prev prev_affine prev_red dW lddw X0 ld0 N0 cf_scratch P C_out C_in "
                             "coef_lazy stream",
}


def base(entry, pooled):
    """A fully valid argument set of `entry` (never passed as it is), every pitch its channel count.  pn2_conv1x1_bwd_cf takes the
    pooled form only and pn2_conv1x1_bwd_first the dense one, whatever `pooled` says."""
    pooled = entry == "pn2_conv1x1_bwd_cf" or (pooled and entry != "pn2_conv1x1_bwd_first")
    co, ci = (128, 64) if entry == "pn2_conv1x1_bwd_cf" else (64, 64) if entry == "pn2_conv1x1_bwd_first" else (64, 32)
    a = dict(dZ=FAKE, ldz=co, dZp=None, ldo=0, arg=None, Kpool=0, Y=FAKE, ldy=co, coef=FAKE, W=FAKE, ldw=ci, prev_Y=FAKE, ld_prev=ci,
             prev_affine=FAKE, dXout=FAKE, ldxo=ci, prev_red=FAKE, X=FAKE, ldx=ci, x_affine=FAKE, dW=FAKE, lddw=ci, dbias=None, P=ROWS,
             C_out=co, C_in=ci, coef_lazy=None, workspace=None, scratch=FAKE, bias=FAKE, X0=FAKE, ld0=12, N0=6, cf_scratch=FAKE,
             stream=None)
    if pooled:
        a.update(dZ=None, ldz=0, dZp=FAKE, ldo=co, arg=FAKE, Kpool=32)
    return a


def lazy_record(over, coef, C):
    from pointnet12_amd import _lib
    f = dict(red=FAKE, gamma=FAKE, affine=FAKE, coef=coef, dgamma=None, dbeta=None, accumulate=0, count=ROWS, C=C)
    f.update(over)
    return _lib.BnCoefLazy(**f)


NINE = ("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad", "pn2_conv1x1_wgrad_ws", "pn2_conv1x1_bwd_pair", "pn2_conv1x1_bwd")
DZ_PITCH = ("pn2_conv1x1_wgrad", "pn2_conv1x1_wgrad_ws")       # (pn2_conv1x1_bwd: ldz must EQUAL ldy, its own rows below)
ALL = NINE + ("pn2_conv1x1_bwd_cf", "pn2_conv1x1_bwd_first")

# (entries, pooled baseline?, what is wrong, overrides, expected code)
TABLE = [
    # one condition of the operand
    (NINE, False, "neither dZ nor dZp", dict(dZ=None), EINVAL),
    (NINE, True, "dZp without arg", dict(arg=None), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "dZp without arg", dict(arg=None), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "no dZp", dict(dZp=None), EINVAL),
    (("pn2_conv1x1_bwd_first",), False, "no dZ", dict(dZ=None), EINVAL),
    (NINE, True, "Kpool 0", dict(Kpool=0), EINVAL),
    (NINE, True, "Kpool negative", dict(Kpool=-32), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "Kpool 0", dict(Kpool=0), EUNSUPPORTED),          # (its group size is a matter of the shape list)
    (("pn2_conv1x1_bwd_cf",), True, "Kpool negative", dict(Kpool=-32), EUNSUPPORTED),
    (NINE + ("pn2_conv1x1_bwd_first",), False, "no Y", dict(Y=None), EINVAL),
    (ALL, False, "no coef", dict(coef=None), EINVAL),
    (DZ_PITCH, False, "ldz % 4", dict(ldz=66), EINVAL),
    (DZ_PITCH, False, "ldz < round4(C_out)", dict(ldz=60), EINVAL),
    (DZ_PITCH + ("pn2_conv1x1_bwd", "pn2_conv1x1_bwd_cf"), True, "ldo % 4", dict(ldo=130), EINVAL),
    (DZ_PITCH + ("pn2_conv1x1_bwd", "pn2_conv1x1_bwd_cf"), True, "ldo < round4(C_out)", dict(ldo=60), EINVAL),
    (NINE + ("pn2_conv1x1_bwd_first",), False, "ldy % 4", dict(ldy=66, ldz=66), EINVAL),
    (NINE + ("pn2_conv1x1_bwd_first",), False, "ldy < round4(C_out)", dict(ldy=60, ldz=60), EINVAL),
    (NINE, True, "ldy % 4, pooled", dict(ldy=66), EINVAL),
    (ALL, False, "P 0", dict(P=0), EINVAL),
    (ALL, False, "P 2^31", dict(P=1 << 31), EINVAL),
    (NINE + ("pn2_conv1x1_bwd_cf",), True, "P 0, pooled", dict(P=0), EINVAL),
    (NINE + ("pn2_conv1x1_bwd_cf",), True, "P 2^31, pooled", dict(P=1 << 31), EINVAL),
    (("pn2_conv1x1_bwd", "pn2_conv1x1_bwd_first"), False, "ldz != ldy", dict(ldz=68), EINVAL),
    (("pn2_conv1x1_bwd",), True, "Kpool no power of two", dict(Kpool=48), EINVAL),
    (("pn2_conv1x1_bwd",), True, "P % Kpool", dict(P=ROWS + 16), EINVAL),
    (("pn2_conv1x1_bwd",), True, "pooled without prev_affine", dict(prev_affine=None, prev_red=None), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "scratch not 256-byte aligned", dict(scratch=FAKE + 16), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "dZp not 16-byte aligned", dict(dZp=FAKE + 4), EINVAL),
    (("pn2_conv1x1_bwd_first",), False, "cf_scratch not 16-byte aligned", dict(cf_scratch=FAKE + 8), EINVAL),
    (ALL, False, "lazy record with a null coef", dict(coef_lazy=dict(coef=None)), EINVAL),
    (ALL, False, "lazy record and no coef", dict(coef=None, coef_lazy=dict(coef=FAKE)), EINVAL),
    (ALL, False, "lazy record for another block", dict(coef_lazy=dict(coef=FAKE + 4096)), EINVAL),
    (ALL, False, "lazy record with another C", dict(coef_lazy=dict(C=32)), EINVAL),
    (ALL, False, "lazy record without reductions", dict(coef_lazy=dict(red=None)), EINVAL),
    # a sound operand on a shape the entry point does not have
    (("pn2_conv1x1_bwd_cf",), True, "C_in 32", dict(C_in=32, ldw=32, ld_prev=32, ldxo=32, lddw=32), EUNSUPPORTED),
    (("pn2_conv1x1_bwd_first",), False, "C_out 128", dict(C_out=128, ldy=128, ldz=128), EUNSUPPORTED),
    (("pn2_conv1x1_bwd_first",), False, "P % 64", dict(P=ROWS + 32), EUNSUPPORTED),
    # two at once: which one wins
    (NINE, True, "Kpool 0 and ldy % 4", dict(Kpool=0, ldy=66), EINVAL),
    (NINE, False, "no dZ and P 2^31", dict(dZ=None, P=1 << 31), EINVAL),
    (("pn2_conv1x1_bwd",), False, "ldz != ldy and C_out % 32", dict(ldz=68, C_out=48, ldy=48), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "misaligned scratch on a shape it does not have", dict(scratch=FAKE + 16, C_in=32, ldw=32, ld_prev=32, ldxo=32, lddw=32), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "ldo % 4 with Kpool 0", dict(ldo=130, Kpool=0), EINVAL),
    (("pn2_conv1x1_bwd_cf",), True, "lazy record with a null coef on a shape it does not have", dict(coef_lazy=dict(coef=None), C_in=32, ldw=32, ld_prev=32, ldxo=32, lddw=32), EINVAL),
    (("pn2_conv1x1_bwd_first",), False, "ldz != ldy with P % 64", dict(ldz=68, P=ROWS + 32), EINVAL),
    (("pn2_conv1x1_bwd_first",), False, "misaligned cf_scratch with C_out 128", dict(cf_scratch=FAKE + 8, C_out=128, ldy=128, ldz=128), EINVAL),
    (("pn2_conv1x1_bwd_first",), False, "N0 13 with P 0", dict(N0=13, P=0), EINVAL),
]

CASES = [pytest.param(e, pooled, over, want, id="%s-%s" % (e[len("pn2_conv1x1_"):], what.replace(" ", "_")))
         for entries, pooled, what, over, want in TABLE for e in entries]


def run(entry, pooled, over):
    from pointnet12_amd import _lib
    a = base(entry, pooled)
    a.update(over)
    keep = None
    if isinstance(a["coef_lazy"], dict):
        keep = lazy_record(a["coef_lazy"], a["coef"], a["C_out"])
        a["coef_lazy"] = ctypes.addressof(keep)
    return getattr(_lib.load(), entry)(*[a[n] for n in ORDER[entry].split()])


@pytest.mark.parametrize("entry,pooled,over,want", CASES)
def test_bad_operand_is_refused_before_any_launch(entry, pooled, over, want):
    assert run(entry, pooled, over) == want


def test_the_table_names_every_argument_of_the_binding():
    from pointnet12_amd import _lib
    for entry, names in ORDER.items():
        assert len(names.split()) == len(_lib.SIGNATURES[entry][1]), entry
