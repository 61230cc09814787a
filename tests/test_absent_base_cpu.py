"""What every launcher answers to a tensor reference into an absent base - no GPU: the library validates on the host.

One record per stage kind and tensor slot (all 289 slots of opdefs.OPS): valid dims, every other slot inside a bound CPU tensor, the
slot under test inside a base that is not bound, under the flags and fields with which the launcher reads that slot.  Every one of
them is refused before a launch, with the code and text below (recorded from the library before the launchers shared one resolver)."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D

EFAULT, EINVAL, EHIP = -14, -22, -5
FOLD = dict(FCOUNT=128, FNREP=1, FEPS=1e-3, FMOM=0.1)
DW = dict(B=2, C=4, H=8, W=8, K=3, STRIDE=1, PAD_T=1, PAD_L=1, HO=8, WO=8, PRO=D.PRO_SILU)
PLANE = dict(B=2, C=4, HW=64)
PATCH = dict(B=1, C=2, T=1, H=8, W=8, P=4, TUB=1)
RECOMPUTE = dict(COEF=None, ACT=D.ACT_SILU)        # BN_BWD_APPLY reads MULBC / ADDBC / PS only without a COEF table

# kind -> (fields of a valid record, {slot: fields that differ while that slot is the one under test})
# (WGRAD has no kernel for an SE gate on P: a record whose GATEP is bound is turned down later, but its references are resolved and
# answered first, like every other slot's)
SPEC = {
    "MEMSET": (dict(BYTES=16), {}),
    "AXPY": (dict(COUNT=16), {}),
    "WEIGHT_PACK": (dict(TOTAL=8192, N_ENTRIES=1), {}),
    "CONV": (dict(B=1, C1=8, C2=8, H=8, W=8, M=8, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=8, WO=8, PRO1=D.PRO_SILU, PRO2=D.PRO_AFFINE,
                  MODE=D.MODE_CONV, W_SM=1, W_SK=128, W_ST=128, FLIP=0, BETA=0, YC=8, NREP=1, X1_BF16=0),
             {"WTB": dict(_flags=D.FLAG_BF16)}),
    "WGRAD": (dict(B=1, M=8, C=8, CTOT=8, H=8, W=8, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=8, WO=8, PROP=D.PRO_NONE, PROQ=D.PRO_SILU,
                   MODE=D.MODE_CONV, P_BF16=0), {}),
    "WGRAD_FINALIZE": (dict(TOTAL=64, N_ENTRIES=1), {}),
    "DWCONV_FWD": (dict(DW, NREP=1, **FOLD), {}),
    "DWCONV_DGRAD": (dict(DW, BETA=0, NREP=1), {}),
    "DWCONV_WGRAD": (dict(DW), {}),
    "BN_FINALIZE": (dict(COUNT=128, C=4, TRAIN=1, NREP=1, EPS=1e-3, MOM=0.1), {}),
    "SE_POOL": (dict(PLANE, PRO=D.PRO_SILU, **FOLD), {}),
    "SE_FC": (dict(B=2, C=4, CSQ=2), {}),
    "SE_FC_BWD": (dict(B=2, C=4, CSQ=2), {}),
    "SE_BWD_REDUCE": (dict(PLANE, PRO=D.PRO_SILU), {}),
    "BN_BWD_REDUCE": (dict(PLANE, ACT=D.ACT_SILU, NREP=1, KEEP=0.8, ADDSCALE=1.0), {}),
    "BN_BWD_FINALIZE": (dict(COUNT=128, C=4, NREP=1), {}),
    "BN_BWD_APPLY": (dict(PLANE, NREP=1, ACT=D.ACT_NONE, EVAL=0, OUT_BF16=0, COUNT=128, ADDSCALE=1.0),
                     {"MULBC": RECOMPUTE, "ADDBC": RECOMPUTE, "PS": RECOMPUTE}),
    "BN_RESIDUAL": (dict(PLANE, KEEP=0.8, **FOLD), {}),
    "CHANNEL_SUM": (dict(PLANE), {}),
    "LOSS_FWD": (dict(B=1, C=4, HW=64, MODE=0, IGNORE=0, REDUCE_SUM=0, GAMMA=2.0, SMOOTH=0.0), {}),
    "LOSS_BWD": (dict(B=1, C=4, HW=64, MODE=0, IGNORE=0, REDUCE_SUM=0, GAMMA=2.0, SMOOTH=0.0), {}),
    "ARGMAX": (dict(B=1, C=4, HW=64), {}),
    "CHAN_LN_FWD": (dict(B=1, C=8, HW=16, EPS=1e-6), {}),
    "CHAN_LN_BWD": (dict(B=1, C=8, HW=16, ACCUM=1), {}),
    "ACT_BWD": (dict(COUNT=16, ACT=D.ACT_SILU), {}),
    "ACT_FWD": (dict(COUNT=32, ACT=D.ACT_SILU, C=4, HW=4), {}),
    "ATTN_FWD": (dict(B=1, HEADS=1, HD=8, L=8, LS=8, SCALE=0.35), {}),
    "ATTN_BWD": (dict(B=1, HEADS=1, HD=8, L=8, LS=8, SCALE=0.35), {}),
    "MAE_MASK_INDEX": (dict(B=1, L=16, KEEP=4), {}),
    "IDS_TO_DEC_IDX": (dict(B=1, L=16, KEEP=4), {}),
    "TOKEN_GATHER": (dict(B=1, C=4, LIN=8, LOUT=8, POS_BY_SRC=0, POS_OFF=0, LIN_S=8, LOUT_S=8), {}),
    "TOKEN_SCATTER": (dict(B=1, C=4, LIN=8, LOUT=8, LIN_S=8, LOUT_S=8), {}),
    "PATCHIFY": (dict(PATCH, INVERSE=0, ORDER=0, LS=0, L_OFF=0), {"IMGS": dict(INVERSE=4, ORDER=1)}),
    "MAE_LOSS_FWD": (dict(PATCH, LP=4, L_OFF=0, NORM_PIX=0), {}),
    "MAE_LOSS_BWD": (dict(PATCH, LP=4, L_OFF=0, NORM_PIX=0), {}),
    "TRANSPOSE_CL": (dict(B=1, C=4, L=8, L_OFF=0, LOUT=8, YS=0, Y_OFF=0), {}),
    "CONFUSION": (dict(COUNT=16, C=4), {}),
    "DROP_GATE": (dict(COUNT=16, P=0.5), {}),
    "TILE_PREP": (dict(B=1, C=2, H=8, W=8, S=4, NSRC=1), {}),
    "SE_BN_SUMS": (dict(PLANE, ACT=D.ACT_SILU), {}),
    "SE_BN_COMBINE": (dict(B=2, C=4, ADDSCALE=1.0), {}),
    "SPACE_TO_DEPTH": (dict(B=1, C=2, H=4, W=4), {}),
    "UPSAMPLE_ZERO": (dict(B=1, C=2, H=4, W=4, S=2, HO=8, WO=8), {}),
    "SE_FC_WGRAD": (dict(B=2, C=4, CSQ=2), {}),
    "IM2COL": (dict(B=1, C=2, H=8, W=8, KH=3, KW=3, STRIDE=2, PAD_T=0, PAD_L=0, HO=4, WO=4), {}),
    "TILE_LABEL_HIST": (dict(M=1, H=8, W=8, K=4, Y0=0, X0=0, WH=8, WW=8, NSRC=1), {}),
    "TILE_MOMENTS": (dict(M=2, C=2, H=8, W=8, NSRC=2, NB=1), {}),
    "WINDOW_BLEND": (dict(M=1, F=1, NY=1, NX=1, K=4, H=8, W=8, S=8, NSRC=1, MODE=0), {}),
    "SEG_STATS": (dict(P=1, NC=1), {}),
    "SEG_HIST": (dict(P=1, NC=1, NB=16), {}),
    "GRAD_CLIP": (dict(P=1, NC=1, APPLY=1, MAX_NORM=1.0), {}),
    "TILE_RADIX_HIST": (dict(M=2, C=3, H=8, W=8, NSRC=2, NBND=3, POOLED=0, PASS=1, R=4), {}),
    "TILE_RANK_PICK": (dict(N=192, G=2, R=4, STEP=1), {}),
    "TILE_QUICKLOOK": (dict(B=2, C=3, H=8, W=8, SH=4, SW=4, NSRC=2, NROW=2, NQ=2), {}),
    "CLASS_OVERLAY": (dict(B=2, SH=4, SW=4, K=4, ALPHA=128, SKIP0=0), {}),
}

ABSENT = "GRADS"         # a base that is never bound (index 2)
STRIDE = 8192            # bytes between the slots of a record inside the bound base: no two tensors alias

# kind -> (code, text after "op 0 (KIND): ") for every slot of the kind; EXCEPT names the slots that answer differently
ANSWER = {kind: (EFAULT, f"{kind.lower()}: tensor references a null base") for kind in D.OPS}
ANSWER.update({
    "MEMSET": (EFAULT, "memset: null base 2"),
    "DWCONV_FWD": (EFAULT, "dwconv_fwd: null base"),
    "DWCONV_DGRAD": (EFAULT, "dwconv_dgrad: null base"),
    "DWCONV_WGRAD": (EFAULT, "dwconv_wgrad: null base"),
    "LOSS_FWD": (EFAULT, "loss_fwd: null base"),
    "LOSS_BWD": (EFAULT, "loss_bwd: null base"),
    "ARGMAX": (EFAULT, "argmax: null base"),
    "CONFUSION": (EFAULT, "confusion: null base"),
    "ATTN_FWD": (EINVAL, "attn_fwd: missing tensor or null base"),
    "ATTN_BWD": (EINVAL, "attn_bwd: missing tensor or null base"),
})
EXCEPT = {kind: {name: (EINVAL, f"{kind.lower()}: folded BN_FINALIZE needs FSTATS, FGAMMA, FBETA, FRM, FRV") for name in D.FOLD_T}
          for kind in D.FOLD_KINDS}


def _launch(kind, absent_slot):
    """(code, message) of one record of `kind` over a bound CPU workspace, slot `absent_slot` (None = none) inside an unbound base"""
    from s2lc_amd import _lib
    from s2lc_amd.plan.program import Program, TRef

    fields, per_slot = SPEC[kind]
    f = dict(fields)
    for j, name in enumerate(D.OPS[kind][0]):
        f[name] = TRef(D.BASE[ABSENT if name == absent_slot else "WS"], j * STRIDE, (1,))
    f.update(per_slot.get(absent_slot, {}))
    p = Program()
    p.add(kind, **f)
    ws = torch.zeros(D.N_T * STRIDE, dtype=torch.uint8)
    bases = _lib.Bases().set("WS", ws)
    packed = p.pack()
    L = _lib.lib()
    rc = L.s2k_program_run(packed.ctypes.data, 0, 1, bases.ptr, len(D.BASES), 0)
    return rc, L.s2k_last_error().decode()


SLOTS = [(kind, name) for kind, (t, _, _, _) in D.OPS.items() for name in t]


def test_every_slot_of_every_kind_is_covered():
    assert len(D.OPS) == 55 and set(SPEC) == set(D.OPS) and set(ANSWER) == set(D.OPS)
    assert len(SLOTS) == 289 == sum(len(t) for t, _, _, _ in D.OPS.values())
    for kind, (fields, per_slot) in SPEC.items():
        assert set(per_slot) <= set(D.OPS[kind][0]) and set(EXCEPT.get(kind, {})) <= set(D.OPS[kind][0]), kind
        for code, text in [ANSWER[kind], *EXCEPT.get(kind, {}).values()]:
            assert code in (EFAULT, EINVAL) and "HIP" not in text, kind     # refused by the host, never a launch error


@pytest.mark.parametrize("kind", list(D.OPS))
def test_a_reference_into_an_absent_base_is_refused_before_any_launch(kind):
    import __graft_entry__ as g

    g.build()
    for name in D.OPS[kind][0]:
        code, text = EXCEPT.get(kind, {}).get(name, ANSWER[kind])
        rc, msg = _launch(kind, name)
        print(kind, name, rc, msg)
        assert rc != EHIP and "HIP" not in msg, (kind, name, "reached a launch")
        assert (rc, msg) == (code, f"op 0 ({kind}): {text}"), (kind, name)
