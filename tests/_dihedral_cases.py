"""Cases, restatement and checker of the rot90 / flip augmentation kernel (tsr_gather_dihedral, csrc/dihedral.hip).

The restatement is the contract composed from torch ops -- ``index_select``, ``flip``, ``rot90``, the channel map, the
scale -- written without reading ``tactilesr_amd.functional``.  The transform moves bits, so the checker compares int32
views: a NaN must arrive with its payload, at its mapped position only.
"""
import ctypes

import torch

OPS = tuple(range(8))
EVEN_OPS = (0, 2, 4, 6)
NAN_BITS = 0x7fc00000

# (C, H, W): why the shape is in the table
SHAPES = [
    ((3, 4, 4), "the taxel planes: the one-thread-per-element path"),
    ((24, 4, 4), "the Seqs taxels: 24 channels on the small path"),
    ((1, 1, 1), "a one-element plane: every op is the identity"),
    ((1, 40, 40), "the SR target of the project: one full tile and a ragged 8-wide one, float4 rows"),
    ((1, 100, 100), "the depth map: 100 = 3 * 32 + 4, a ragged last tile of one float4"),
    ((1, 124, 124), "the scale-factor 31 target: 124 = 3 * 32 + 28"),
    ((1, 64, 64), "whole tiles only"),
    ((1, 65, 65), "one element past a tile edge, odd pitch: the one-float-per-lane path"),
    ((2, 33, 33), "odd pitch and two planes: plane bases at odd offsets"),
    ((1, 132, 132), "past the one-workgroup-per-plane limit (H (W + 1) dwords in 62 KiB): 64x64 tiles, float4 rows, ragged by 4"),
    ((1, 129, 129), "the tile path at an odd pitch: one float per lane, one element past two tiles"),
    ((1, 8, 8), "64 elements: the largest plane of the small path"),
    ((1, 9, 9), "81 elements: the smallest square plane past the small path"),
    ((1, 125, 125), "125 * 126 dwords: the largest square plane one workgroup stages"),
    ((1, 126, 126), "126 * 127 dwords: the smallest square plane that goes as tiles"),
]
NONSQUARE = [
    ((3, 5, 7), "non-square small planes, even k only"),
    ((1, 31, 65), "non-square, even k only, odd pitch"),
    ((1, 36, 500), "non-square on the tile path (36 x 501 dwords do not fit): 8 tiles along a row, the last ragged"),
]
PLANE_LDS_DWORDS = 15872                  # DH_PLANE_LDS of csrc/dihedral.hip: the threshold between the two kernels


def path_of(shape):
    """Which kernel a (C, H, W) shape takes: the threshold cases of the tables must sit on both sides."""
    _, H, W = shape
    return "small" if H * W <= 64 else ("plane" if H * (W + 1) <= PLANE_LDS_DWORDS else "tile")
BATCHES = (1, 7, 67)
INDEX_KINDS = ("none", "perm", "reversed", "repeats")
OFFSETS = (1, 2, 3)                       # floats: src and out bases off 16-byte alignment
MANY = (2100, (1, 40, 40))                # 2100 planes: several rounds of resident workgroups, every sample distinct
# (max_wgs, why): tsr_gather_dihedral_wgs launches at most max_wgs workgroups and each walks the further work items
WALKS = [(1, "one workgroup walks every item: lds is rewritten after every transposing item"),
         (3, "a stride that divides no item count of the tables: the last round is ragged"),
         (1 << 20, "the default cap: no walk at these sizes")]
SCALES = (1.0, 0.125, -0.25, 0.0)


def plane_op(x, op):
    """op = k + 4 f on the last two dimensions: mirror along W when f, then k counter-clockwise quarter turns."""
    if op >= 4:
        x = x.flip(-1)
    return torch.rot90(x, op % 4, (-2, -1))


def axis_tables(C, axis_cnt=3):
    """The vector axis mode written out from the geometry: with (r, c) -> (i, j) the op's coordinate map, the in-plane
    force (along +H, along +W) of a group transforms with the map's 2x2 matrix M, everything else stays.  M is read off
    a probe: where the unit steps along r and along c of a 3x3 index image land."""
    n = 3
    grid = torch.arange(n * n, dtype=torch.float32).view(1, 1, n, n)
    cmap = torch.arange(C, dtype=torch.int32).repeat(8, 1)
    csign = torch.ones(8, C, dtype=torch.float32)
    for op in OPS:
        out = plane_op(grid, op)[0, 0]
        pos = {int(out[i, j]): (i, j) for i in range(n) for j in range(n)}
        o, dr, dc = pos[0], pos[n], pos[1]                         # images of (0,0), (1,0), (0,1)
        M = [[dr[0] - o[0], dc[0] - o[0]], [dr[1] - o[1], dc[1] - o[1]]]      # columns: image of e_r, of e_c
        for g in range(0, C, axis_cnt):
            for row in range(2):                                   # output component `row` = sum_k M[row][k] * source k
                k = 0 if M[row][0] != 0 else 1
                cmap[op, g + row] = g + k
                csign[op, g + row] = float(M[row][k])
    return cmap, csign


def det(op):
    n = 3
    out = plane_op(torch.arange(n * n, dtype=torch.float32).view(n, n), op)
    pos = {int(out[i, j]): (i, j) for i in range(n) for j in range(n)}
    o, dr, dc = pos[0], pos[n], pos[1]
    return (dr[0] - o[0]) * (dc[1] - o[1]) - (dc[0] - o[0]) * (dr[1] - o[1])


def restate(src, ops, index=None, tables=None):
    """D_{ops[b]}(src[index[b]]) per sample, bit-moving only (a negative sign is torch's neg: the sign bit).  ``ops`` is a
    list of ints, one per output sample."""
    sel = src if index is None else src.index_select(0, torch.as_tensor(index, dtype=torch.long, device=src.device))
    out = []
    for b, op in enumerate(ops):
        x = sel[b]
        if tables is not None:
            cmap, csign = tables
            x = x.index_select(0, cmap[op].long().to(x.device))
            neg = (csign[op] < 0).view(-1, 1, 1).to(x.device)
            x = torch.where(neg, -x, x)
        out.append(plane_op(x, op))
    return torch.stack(out).contiguous()


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    bad = (g != w)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def make_src(n, shape, seed):
    """Distinct finite values: element e of the tensor holds a value no other element holds (a wrong source position
    cannot pass), with both signs."""
    C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    total = n * C * H * W
    v = (torch.randperm(total, generator=g).float() - total // 2) * 0.25 + 0.125
    return v.view(n, C, H, W)


def make_index(kind, B, n_src, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return None
    if kind == "perm":
        return torch.randperm(n_src, generator=g)[:B].clone()
    if kind == "reversed":
        return torch.arange(n_src - 1, -1, -1)[:B].clone()
    if kind == "repeats":
        return torch.randint(0, max(1, n_src // 2), (B,), generator=g)
    raise ValueError(kind)


def make_ops(B, allowed, seed):
    """Every allowed op present when B allows, the rest drawn."""
    g = torch.Generator().manual_seed(seed)
    ops = [allowed[int(k)] for k in torch.randint(0, len(allowed), (B,), generator=g)]
    for k, op in enumerate(allowed[:B]):
        ops[(k * 3) % B if B > 3 * len(allowed) else k] = op       # B = 67: spread over the batch (3 k < 67: no collision)
    return ops


def mask_of(ops):
    m = 0
    for o in ops:
        m |= 1 << o
    return m


# ---- refusals: (label, overrides of BASE_ARGS); pointers: 1 = given, 0 = NULL
BASE_ARGS = dict(src=1, n_src=8, idx=1, op=1, op_all=0, op_mask=0xff, cmap=0, csign=0, out=1, B=4, C=3, H=4, W=4,
                 scale=1.0, accumulate=0)
REFUSALS = [
    ("null src", dict(src=0)), ("null out", dict(out=0)),
    ("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("n_src 0", dict(n_src=0)), ("n_src -3", dict(n_src=-3)),
    ("C 0", dict(C=0)), ("C -1", dict(C=-1)), ("H 0", dict(H=0)), ("H -4", dict(H=-4)), ("W 0", dict(W=0)), ("W -4", dict(W=-4)),
    ("op_mask 0", dict(op_mask=0)), ("op_mask bit 8", dict(op_mask=0x100)), ("op_mask 0x1ff", dict(op_mask=0x1ff)),
    ("op_mask -1", dict(op_mask=-1)),
    ("odd k, H != W", dict(H=5, W=7, op_mask=0x02)), ("odd k among even, H != W", dict(H=31, W=65, op_mask=0x55 | 0x80)),
    ("all ops, H != W", dict(H=4, W=5)),
    ("op_all outside the mask", dict(op=0, op_all=3, op_mask=0x05)), ("op_all 8", dict(op=0, op_all=8)),
    ("op_all -1", dict(op=0, op_all=-1)),
    ("cmap without csign", dict(cmap=1)), ("csign without cmap", dict(csign=1)),
    ("C*H*W = 2^31", dict(C=1 << 11, H=1 << 10, W=1 << 10)), ("C*H*W above 2^31, small plane", dict(C=(1 << 31) - 1, H=2, W=2)),
    ("C*H*W wraps 32 bits", dict(C=1 << 16, H=1 << 16, W=1 << 16, op_mask=0x55)),
    ("max_wgs 0", dict(max_wgs=0)), ("max_wgs -1", dict(max_wgs=-1)), ("null src through _wgs", dict(max_wgs=4, src=0)),
    ("odd k, H != W through _wgs", dict(max_wgs=4, H=5, W=7, op_mask=0x02)),
    ("accumulate 2", dict(accumulate=2)), ("accumulate -1", dict(accumulate=-1)), ("scale NaN", dict(scale=float("nan"))),
]
ADDR = dict(src=4096, idx=8192, op=12288, cmap=16384, csign=20480, out=24576)


def call_raw(lib, a, stream=0, **ptrs):
    """tsr_gather_dihedral with the scalars of ``a`` (tsr_gather_dihedral_wgs when ``a`` holds ``max_wgs``); a pointer is
    ``ptrs[name]`` when given, else the small fake address ADDR[name] nothing may dereference (a[name] = 1) or NULL
    (a[name] = 0).  Returns the status."""
    P = ctypes.c_void_p

    def p(name):
        return P(ptrs[name] if name in ptrs else (ADDR[name] if a[name] else 0))
    head = (p("src"), a["n_src"], p("idx"), p("op"), a["op_all"], a["op_mask"], p("cmap"), p("csign"), p("out"), a["B"], a["C"],
            a["H"], a["W"], ctypes.c_float(a["scale"]), a["accumulate"])
    if "max_wgs" in a:
        return lib.tsr_gather_dihedral_wgs(*head, a["max_wgs"], P(stream))
    return lib.tsr_gather_dihedral(*head, P(stream))
