"""Case tables and fp64 references of tests/test_gpu_architectures.py: TactileSR across stem counts (T = seqsCnt) and block
counts (M = MSRBs, R = ResBlocks).  Everything here runs without a GPU (no device import at module level);
tests/test_arch_cases_cpu.py checks that every case is a sound test: finite, live output, images of one magnitude, a ReLU
pattern that is neither dead nor saturated, and -- for the dominance cases -- that the copied half of the head's input really
dominates.

All cases: scale_factor 3 (12 x 12 image = 2 x 2 ragged 8 x 8 tiles) and B = 3 unless noted (odd: absent image slots in the
2- and 4-image workgroups).  Weights `O.random_state_dict(O.tactilesr_state_shapes(**cfg), seed)`, taxels rand * 8, target
rand * 25 (`_gradcheck.step_data`).

EVAL   id   T  M  R   why
       e1   3  1  1   fuse conv C_in 192: odd number of 64-blocks
       e2   4  1  2   first R > 1: ping-pong of the force branch, one swap
       e3   5  2  1   C_in 320
       e4   6  1  3   R = 3: two swaps, the result lands from `f0`
       e5   9  1  1   C_in 576, beyond every kernel test
       e6  10  3  2   C_in 640; odd M
       e7   1  0  1   M = 0: the fuse output is copied into channels [64, 128) of the head's input
       e8   2  1  0   R = 0: the force stem is copied into channels [0, 64)
       e9   1  0  0   both copies: no conv ever writes the max|.| slot of the head's input
       e10  3  0  2   copy path + ping-pong

DOMINANCE (the copied half of the head's input dominates the other; everything else as drawn)
       d1 = e7, inputContact_layer.1.{weight,bias} x 64       max|fuse| / max|force| >= 16
       d2 = e8, input_layer_force.1.weight x 64               max|force_in| / max|msrb0| >= 16
       d3 = e9, inputContact_layer.1.{weight,bias} x 2^14     max|fuse| > 2 * 65504 (a max|.| slot of 0 means scale 1: only
                                                              values beyond fp16's range overflow)
  The fp16x3 head conv scales its input by 2^(13 - floor(log2 in_amax)): a half more than 8x above in_amax leaves the fp16
  range.  Plain random cases keep the two halves within ~2.5x of each other and cannot see a missing bound.

TRAIN  t1 (3,1,2) B 1, 3   t2 (4,2,1) B 3   t3 (5,1,3) B 1, 3   t4 (6,1,1) B 3   t5 (9,1,2) B 3

Bars.  Eval: TOL = 1e-5 of the output maximum; e5 / e6 (K = 5184 / 5760 in the fuse conv): max(1e-5, 4 * e_ref), e_ref = the
error of torch's own fp32 CPU forward of the same case against fp64 (the rule and the margin of tests/_wgrad_check.py).
e_ref as measured on the CPU (tests/test_arch_cases_cpu.py prints it):
       e5  6.5e-07      e6  1.1e-06          -> 4 * e_ref < 1e-5: both bars are the flat 1e-5
"""
import functools

import torch

from oracle import tactilesr_oracle as O
import _gradcheck as GC

TOL = 1e-5
SF = 3
B = 3

EVAL = {"e1": (3, 1, 1), "e2": (4, 1, 2), "e3": (5, 2, 1), "e4": (6, 1, 3), "e5": (9, 1, 1), "e6": (10, 3, 2),
        "e7": (1, 0, 1), "e8": (2, 1, 0), "e9": (1, 0, 0), "e10": (3, 0, 2)}
# id -> (base case, {state_dict key: factor}, (numerator stage, denominator stage or None, bound))
DOMINANCE = {
    "d1": ("e7", {"inputContact_layer.1.weight": 64.0, "inputContact_layer.1.bias": 64.0}, ("fuse", "force", 16.0)),
    "d2": ("e8", {"input_layer_force.1.weight": 64.0}, ("force_in", "msrb0", 16.0)),
    "d3": ("e9", {"inputContact_layer.1.weight": 2.0 ** 14, "inputContact_layer.1.bias": 2.0 ** 14},
           ("fuse", None, 2 * 65504.0)),
}
TRAIN = {"t1": (3, 1, 2), "t2": (4, 2, 1), "t3": (5, 1, 3), "t4": (6, 1, 1), "t5": (9, 1, 2)}
TRAIN_B = {"t1": (1, 3), "t2": (3,), "t3": (1, 3), "t4": (3,), "t5": (3,)}

EVAL_IDS = list(EVAL) + list(DOMINANCE)
FULL = [c for c in EVAL if min(EVAL[c][1:]) >= 1]             # e1 .. e6: at least one MSRB and one ResBlock
COPY = [c for c in EVAL_IDS if c not in FULL]                 # e7 .. e10, d1 .. d3
WIDE = ("e5", "e6")                                           # bar max(TOL, 4 * e_ref)
TRAIN_CASES = [(c, b) for c in TRAIN for b in TRAIN_B[c]]
SEED = {c: 9100 + 17 * i for i, c in enumerate(list(EVAL) + list(TRAIN))}
# seeds chosen on the CPU conditions alone (tests/test_arch_cases_cpu.py): the first of 9300, 9301, .. that meets them and
# is not in use
SEED["e7"] = 9300        # (the lattice seed left one image of e7 all zero)
SEED["e9"] = 9303        # (d3: the first with max|fuse| > 2 * 65504)
# conditioning: a case under the flat bar must have 4 * e_ref <= TOL, i.e. the rule of e5 / e6 would give it the same bar.
# The lattice seeds of e2 and e3 gave the two worst-conditioned networks of the table, e_ref 3.6e-06 and 5.5e-06 (e2: image
# maximum 2.2 after cancellation in the head) against 0.4 .. 2.1e-06 everywhere else; on such a case 1e-5 is tighter than
# 4x the error of torch's own fp32 forward, and fp32-grade arithmetic lands on either side of it.
SEED["e2"] = 9301        # e_ref 7.3e-07
SEED["e3"] = 9302        # e_ref 1.5e-06


def cfg_of(T, M, R):
    return dict(scale_factor=SF, seqsCnt=T, patternFeatureExtraLayerCnt=M, forceFeatureExtraLayerCnt=R)


def case_cfg(cid):
    base = DOMINANCE[cid][0] if cid in DOMINANCE else cid
    return cfg_of(*(EVAL[base] if base in EVAL else TRAIN[base]))


def train_seed(cid, b):
    return SEED[cid] + b


@functools.lru_cache(maxsize=None)
def case_data(cid, b=B):
    """(cfg, state dict, taxels, target) of an eval, dominance or train case.  Shared, never modified."""
    cfg = case_cfg(cid)
    if cid in TRAIN:
        return (cfg,) + GC.step_data(cfg, b, train_seed(cid, b))
    base = DOMINANCE[cid][0] if cid in DOMINANCE else cid
    sd, LR, HR = GC.step_data(cfg, b, SEED[base])
    if cid in DOMINANCE:
        sd = {k: (v * DOMINANCE[cid][1][k] if k in DOMINANCE[cid][1] else v) for k, v in sd.items()}
    return cfg, sd, LR, HR


def _forward(sd, LR, dtype, stages=None):
    with torch.no_grad():
        return O.tactilesr_forward({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, LR.to(dtype),
                                   scale_factor=SF, stages=stages)


@functools.lru_cache(maxsize=None)
def eval_ref(cid):
    """(fp64 oracle output, its `stages`) of an eval or dominance case."""
    _, sd, LR, _ = case_data(cid)
    stages = {}
    return _forward(sd, LR, torch.float64, stages), stages


@functools.lru_cache(maxsize=None)
def e_ref(cid):
    """Error of torch's fp32 CPU forward of the case against the fp64 oracle, relative to the output maximum."""
    _, sd, LR, _ = case_data(cid)
    return GC.relerr(_forward(sd, LR, torch.float32), eval_ref(cid)[0])


def eval_bar(cid):
    return max(TOL, 4 * e_ref(cid)) if cid in WIDE else TOL


@functools.lru_cache(maxsize=None)
def train_record(cid, b=B):
    """`oracle_grads(.., record=True)` of the case: fp64 loss, gradients, new statistics and ReLU pre-activations."""
    _, sd, LR, HR = case_data(cid, b)
    return GC.oracle_grads(sd, LR, HR, scale_factor=SF, record=True)


def stage_max(stages, name):
    return float(stages[name].abs().max())
