"""Device-resident batch loader for SR training / evaluation.

The reference feeds ``Trainer_tactileSR`` from ``DataLoader(TactileSRDataset(file), batch_size, shuffle)``
(train/tactileSR_train.py:58-59, utility/load_tactile_dataset.py:39-47): every step moves a host batch to the GPU
(train/tactileSR_train.py:43), 40 KB of HR per sample.  At thousands of samples per second per GPU that copy and the
per-sample ``.item()`` unboxing are the step's host bottleneck, so this loader keeps the whole (LR, HR) set on the
device and yields index-gathered batches with the same ``(LR, HR)`` tuple protocol -- ``train_one_iter`` /
``eval_func`` take it unchanged.  Shuffling follows ``torch.randperm`` under its own generator (a
``RandomSampler``-style fresh permutation per epoch; the order is NOT the reference DataLoader's, whose sampler
draws from the global CPU generator).
"""
from __future__ import annotations

from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch


class DeviceSRLoader:
    """``augment`` (default ``None``: the plain loader, untouched) switches on rot90 / flip augmentation on the device:
    ``"rot90"`` (ops 0..3, the reference's ``augmentData``, utility/raw_data_process.py:57-95), ``"dihedral"`` (ops 0..7)
    or an explicit tuple of ops ``k + 4 f`` (``functional.dihedral``).  Each batch is one ``tsr_gather_dihedral`` launch
    per tensor -- the gather and the transform in one pass -- and both tensors of a pair get the same op.

    * ``augment_mode="random"``: each epoch, after the permutation, one op per sample is drawn uniformly from the set
      with the loader's own generator; the epoch's length is unchanged.
    * ``augment_mode="expand"``: the epoch covers every (sample, op) pair once; virtual index ``j`` is sample
      ``j // n_ops`` under ``ops[j % n_ops]`` -- unshuffled, ``augmentData``'s order without storing the copies -- and
      ``len()`` grows by the factor ``n_ops``.

    ``axis_mode="vector"`` also maps the in-plane force channels of the first tensor
    (``functional.dihedral_axis_tables``); the second tensor, ``(N,H,W)`` or ``(N,C,H,W)``, is always turned plane by
    plane.  ``last_index`` / ``last_ops`` hold the latest augmented batch's device arrays (int64 / int32).  Rank
    sharding stays on the base samples.  The batches carry no autograd graph.

    ``taxel_noise`` (default ``None``: the loader untouched, tensors and generator draws alike) is a
    ``functional.TaxelNoise`` or a dict of its fields: every yielded first tensor then passes through one
    ``functional.taxel_noise`` launch after the gather -- gain drift, Gaussian noise, dead taxels -- and the second tensor
    never does.  The draws come from the launch's counter generator alone (seed ``noise_seed``, default the loader's
    ``seed``; offset = the loader's ``epoch``, 1 during the first pass; id = the sample's index in the epoch's virtual set:
    the sample index, or under ``"expand"`` the ``(sample, op)`` index ``j``), so the permutation and the op draws do not
    change, and the noise of a sample in an epoch depends neither on the batch size nor on where shuffling puts it.  Ids
    count within a rank's shard: give each rank its own ``noise_seed``.

    ``gamma`` (default ``None``: the loader as it was, batches and generator draws alike) is an optional (N,) tensor of
    per-sample mask widths (the datasets' ``alphaBeta[2]``) for the degradation-consistency loss.  It is gathered with
    each batch's sample indices -- plain, shuffled, augmented and ``"expand"`` alike; the dihedral ops leave it alone,
    the taxel centres being mirror-symmetric -- and yielded as a third element, ``(LR, HR, gamma)``, which
    ``train_one_iter`` / ``eval_func`` / ``GraphedTrainStep`` accept.  With it ``last_index`` is also kept by the plain
    loader.

    ``weight`` (default ``None``: the loader as it was, draw for draw) is an optional (N,) tensor of per-sample
    supervision weights ``w >= 0`` (0 = an unlabeled sample whose ``HR`` is a placeholder).  It is gathered with each
    batch's sample indices exactly as ``gamma`` is, and the loader then yields 4-tuples ``(LR, HR, gamma, weight)`` with
    ``gamma`` ``None`` when the loader has none -- the form ``train_one_iter`` / ``eval_func`` / ``GraphedTrainStep``
    accept.  ``last_index`` is kept as with ``gamma``."""

    def __init__(self, LR: torch.Tensor, HR: torch.Tensor, batch_size: int, shuffle: bool = False,
                 drop_last: bool = False, seed: Optional[int] = None, device="cuda",
                 rank: int = 0, world_size: int = 1, augment=None, augment_mode: str = "random",
                 axis_mode: str = "planes", axis_cnt: int = 3, taxel_noise=None, noise_seed: Optional[int] = None,
                 gamma: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None):
        assert LR.shape[0] == HR.shape[0], "LR and HR must hold the same number of samples"
        if weight is not None:
            from .._lib import TactileSRHipError
            weight = torch.as_tensor(weight)
            if weight.dim() != 1 or weight.shape[0] != LR.shape[0]:
                raise TactileSRHipError(f"weight must hold one value per sample, ({LR.shape[0]},), got "
                                        f"{tuple(weight.shape)}")
            weight = weight.float()
        if gamma is not None:
            from .._lib import TactileSRHipError
            gamma = torch.as_tensor(gamma)
            if gamma.dim() != 1 or gamma.shape[0] != LR.shape[0]:
                raise TactileSRHipError(f"gamma must hold one value per sample, ({LR.shape[0]},), got {tuple(gamma.shape)}")
            gamma = gamma.float()
        self._ops = None
        self.last_index = self.last_ops = self._arange = None
        self._noise = None
        if taxel_noise is not None:
            from .. import functional as Fh
            from .._lib import TactileSRHipError
            self._noise = Fh.taxel_noise_spec(taxel_noise)
            if LR.dim() != 4 or LR.dtype != torch.float32 or LR.shape[1] % self._noise.axis_cnt:
                raise TactileSRHipError("taxel noise needs a (N,C,H,W) fp32 first tensor with C a multiple of the spec's "
                                        f"axis_cnt, got {tuple(LR.shape)} {LR.dtype}")
            self.noise_seed = int(noise_seed) if noise_seed is not None else (0 if seed is None else int(seed))
        if augment is not None:
            from .. import functional as Fh
            from .._lib import TactileSRHipError
            self._ops = Fh.dihedral_ops(augment)
            if augment_mode not in ("random", "expand"):
                raise TactileSRHipError(f"augment_mode {augment_mode!r} is not 'random' or 'expand'")
            if axis_mode not in Fh.AXIS_MODES:
                raise TactileSRHipError(f"axis_mode {axis_mode!r} is not one of {Fh.AXIS_MODES}")
            if LR.dim() != 4 or HR.dim() not in (3, 4):
                raise TactileSRHipError("augmentation needs a (N,C,H,W) first tensor and a (N,H,W) or (N,C,H,W) second one, "
                                        f"got {tuple(LR.shape)} and {tuple(HR.shape)}")
            if any(o & 1 for o in self._ops):
                for name, t in (("first", LR), ("second", HR)):
                    if t.shape[-1] != t.shape[-2]:
                        raise TactileSRHipError(f"a quarter turn (odd k) needs square planes; the {name} tensor is "
                                                f"{tuple(t.shape)}")
            self.augment_mode, self.axis_mode = augment_mode, axis_mode
            self._op_mask = Fh.dihedral_op_mask(self._ops)
            self._tables = Fh.dihedral_axis_tables(LR.shape[1], axis_cnt) if axis_mode == "vector" else None
        dev = torch.device(device)
        # shard of the set for this rank (data-parallel training: one process per GPU).  EVERY rank gets the same
        # number of samples -- ceil(n/world), the tail wrapping around to the head like DistributedSampler's padding --
        # so every rank runs the same number of batches per epoch and nobody is left alone in an all-reduce.
        n = LR.shape[0]
        if world_size > 1:
            from ..ddp import equal_shard
            idx = torch.as_tensor(equal_shard(n, rank, world_size), dtype=torch.long)
            LR, HR = LR.index_select(0, idx.to(LR.device)), HR.index_select(0, idx.to(HR.device))
            if gamma is not None:
                gamma = gamma.index_select(0, idx.to(gamma.device))
            if weight is not None:
                weight = weight.index_select(0, idx.to(weight.device))
        self.LR = LR.to(dev).contiguous()
        self.HR = HR.to(dev).contiguous()
        self.gamma = gamma.to(dev).contiguous() if gamma is not None else None
        self.weight = weight.to(dev).contiguous() if weight is not None else None
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(0 if seed is None else int(seed))
        self.epoch = 0
        if self._ops is not None:
            self._ops_t = torch.tensor(self._ops, dtype=torch.int32, device=dev)
            if self._tables is not None:
                self._tables = tuple(t.to(dev) for t in self._tables)

    @classmethod
    def from_entries(cls, entries: List[list], batch_size: int, with_gamma: bool = False, with_weight: bool = False,
                     **kw) -> "DeviceSRLoader":
        """From the generator's in-memory entries (tactilesr_amd.data.depth2tactile.synthesize).  ``with_gamma=True``
        also reads each sample's mask width ``alphaBeta[2]`` (data/SRdataset/depth2tactile.py:114-119) into ``gamma``.
        ``with_weight=True`` builds ``weight``: an entry's own ``"weight"`` when it has one, else 1; an entry without
        ``"HR"`` (a recorded sensor frame) gets a zero ``HR`` of the set's shape and weight 0.  A set in which no entry
        has an ``HR`` is refused (there is no shape to take)."""
        LR = torch.stack([torch.as_tensor(e[0]["LR"]) for e in entries])
        if with_weight:
            from .._lib import TactileSRHipError
            have = [torch.as_tensor(e[0]["HR"]) for e in entries if "HR" in e[0]]
            if not have:
                raise TactileSRHipError("with_weight=True: no entry of the set has an HR (nothing gives the HR shape)")
            blank = torch.zeros_like(have[0])
            HR = torch.stack([torch.as_tensor(e[0]["HR"]) if "HR" in e[0] else blank for e in entries])
            kw["weight"] = torch.tensor([(float(e[0].get("weight", 1.0)) if "HR" in e[0] else 0.0) for e in entries],
                                        dtype=torch.float32)
        else:
            HR = torch.stack([torch.as_tensor(e[0]["HR"]) for e in entries])
        if with_gamma:                           # the third entry of the generator's alphaBeta row is the mask width
            kw["gamma"] = torch.tensor([float(np.asarray(e[0]["alphaBeta"]).reshape(-1)[2]) for e in entries],
                                       dtype=torch.float32)
        return cls(LR, HR, batch_size, **kw)

    @classmethod
    def from_file(cls, path: str, batch_size: int, with_gamma: bool = False, with_weight: bool = False,
                  **kw) -> "DeviceSRLoader":
        """From a dataset file in the reference's on-disk format (an object ``.npy`` of ``{'LR','HR',...}`` dicts)
        written by ``save_dataset``.  Object arrays are pickles: only load files you wrote."""
        arr = np.load(path, allow_pickle=True)
        entries = [[arr[i].item() if arr[i].shape == () else arr[i, 0]] for i in range(len(arr))]
        return cls.from_entries(entries, batch_size, with_gamma=with_gamma, with_weight=with_weight, **kw)

    def __len__(self) -> int:
        n = self._virtual_len()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _identity(self) -> torch.Tensor:
        """0 .. N-1 on the device, built once: what the unshuffled loader's ``last_index`` is a slice of."""
        if self._arange is None:
            self._arange = torch.arange(self.LR.shape[0], device=self.LR.device)
        return self._arange

    def _virtual_len(self) -> int:
        n = self.LR.shape[0]
        return n * len(self._ops) if self._ops is not None and self.augment_mode == "expand" else n

    def _iter_augmented(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        from .. import functional as Fh
        dev, n, n_ops = self.LR.device, self._virtual_len(), len(self._ops)
        order = torch.randperm(n, generator=self._gen, device=dev) if self.shuffle else torch.arange(n, device=dev)
        if self.augment_mode == "expand":
            index, ops = torch.div(order, n_ops, rounding_mode="floor"), self._ops_t[order % n_ops]
        else:
            index = order
            ops = self._ops_t[torch.randint(0, n_ops, (n,), generator=self._gen, device=dev)]
        self.epoch += 1
        epoch = self.epoch
        for i in range(len(self)):
            lo, hi = i * self.batch_size, min(n, (i + 1) * self.batch_size)
            idx, op = index[lo:hi].contiguous(), ops[lo:hi].contiguous()
            self.last_index, self.last_ops = idx, op
            lr = Fh.dihedral(self.LR, op, idx, axis_mode=self.axis_mode, op_mask=self._op_mask, tables=self._tables)
            if self._noise is not None:                                 # the virtual index: (sample, op) pairs differ under "expand"
                Fh.taxel_noise(lr, self._noise, self.noise_seed, epoch, ids=order[lo:hi], out=lr)
            hr = Fh.dihedral(self.HR, op, idx, op_mask=self._op_mask)
            if self.weight is not None:
                yield (lr, hr, self.gamma.index_select(0, idx) if self.gamma is not None else None,
                       self.weight.index_select(0, idx))
            elif self.gamma is not None:
                yield lr, hr, self.gamma.index_select(0, idx)
            else:
                yield lr, hr

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        if self._ops is not None:
            yield from self._iter_augmented()
            return
        if self._noise is not None:
            from .. import functional as Fh
        n = self.LR.shape[0]
        order = torch.randperm(n, generator=self._gen, device=self.LR.device) if self.shuffle else None
        self.epoch += 1
        epoch = self.epoch
        for i in range(len(self)):
            lo, hi = i * self.batch_size, min(n, (i + 1) * self.batch_size)
            if order is None:
                lr, hr = self.LR[lo:hi], self.HR[lo:hi]
                if self._noise is not None:                             # out of place: the set itself stays clean
                    lr = Fh.taxel_noise(lr, self._noise, self.noise_seed, epoch, id_base=lo)
            else:
                idx = order[lo:hi]
                lr, hr = self.LR.index_select(0, idx), self.HR.index_select(0, idx)
                if self._noise is not None:
                    Fh.taxel_noise(lr, self._noise, self.noise_seed, epoch, ids=idx, out=lr)
            if self.weight is not None:
                self.last_index = idx if order is not None else self._identity()[lo:hi]
                pick = (lambda v: v.index_select(0, idx)) if order is not None else (lambda v: v[lo:hi])
                yield lr, hr, (pick(self.gamma) if self.gamma is not None else None), pick(self.weight)
            elif self.gamma is not None:
                self.last_index = idx if order is not None else self._identity()[lo:hi]
                yield lr, hr, (self.gamma.index_select(0, idx) if order is not None else self.gamma[lo:hi])
            else:
                yield lr, hr
