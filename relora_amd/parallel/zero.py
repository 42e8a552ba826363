"""ZeRO-1 optimizer-state sharding (reference `adam_zero` /
ZeroRedundancyOptimizer path, torchrun_main.py:668-675, C8/C9).

Each rank owns a greedy-balanced shard of the trainable params, keeps Adam
state only for its shard (1/W of optimizer memory), steps its shard, and
broadcasts the updated parameters to the other ranks through ONE flat
bf16 buffer per owner rank (few large xGMI transfers instead of hundreds of
small broadcasts).

API parity with `ZeroRedundancyOptimizer`:
* `.optim` exposes the inner optimizer (reference `optimizer_reset` accesses
  `optimizer.optim.state` — training_utils.py:350-352);
* `.consolidate_state_dict()` gathers shard states to rank 0;
* `.state_dict()` (after consolidation, on rank 0) returns a state dict in
  the torch format covering ALL params.
"""

from typing import List

import torch
import torch.distributed as dist

from relora_amd.ops.optim import AdamW


def _dist_active():
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


class ZeroRedundancyAdamW:
    def __init__(self, params, process_group=None, **adamw_kwargs):
        self.all_params: List[torch.nn.Parameter] = [p for p in params]
        self.process_group = process_group
        self.world_size = dist.get_world_size(process_group) if _dist_active() else 1
        self.rank = dist.get_rank(process_group) if _dist_active() else 0

        # greedy balance by numel: biggest params first onto the lightest rank
        order = sorted(range(len(self.all_params)),
                       key=lambda i: -self.all_params[i].numel())
        loads = [0] * self.world_size
        self.owner = [0] * len(self.all_params)
        for i in order:
            r = loads.index(min(loads))
            self.owner[i] = r
            loads[r] += self.all_params[i].numel()

        self._param_index = {id(p): i for i, p in enumerate(self.all_params)}
        self.shard_params = [p for p, o in zip(self.all_params, self.owner) if o == self.rank]
        self.optim = AdamW(self.shard_params if self.shard_params else
                           [torch.nn.Parameter(torch.zeros(1))], **adamw_kwargs)
        self._have_params = bool(self.shard_params)
        if self._have_params:
            # stochastic-rounding counters use the position among ALL params,
            # so the drawn bits do not depend on the world size
            self.optim.set_ordinals([self._param_index[id(p)] for p in self.shard_params])

        # flat broadcast buffers, one per owner rank
        self._rank_params = [
            [p for p, o in zip(self.all_params, self.owner) if o == r]
            for r in range(self.world_size)
        ]
        self._flat = None
        self._consolidated = None

    # -- torch.optim-compatible surface ------------------------------------
    @property
    def param_groups(self):
        return self.optim.param_groups

    @property
    def state(self):
        # parity with ZeroRedundancyOptimizer: .state is not the real state
        # (reference comment training_utils.py:316-318); use .optim.state
        return {}

    def zero_grad(self, set_to_none=True):
        for p in self.all_params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        loss = self.optim.step(closure) if self._have_params else None
        if _dist_active():
            self._broadcast_params()
        return loss

    def _ensure_flat(self):
        if self._flat is None:
            self._flat = []
            for r in range(self.world_size):
                numel = sum(p.numel() for p in self._rank_params[r])
                if numel == 0:
                    self._flat.append(None)
                    continue
                p0 = self._rank_params[r][0]
                self._flat.append(torch.empty(numel, dtype=p0.dtype, device=p0.device))

    @torch.no_grad()
    def _broadcast_params(self):
        self._ensure_flat()
        handles = []
        for r in range(self.world_size):
            flat = self._flat[r]
            if flat is None:
                continue
            if r == self.rank:
                off = 0
                for p in self._rank_params[r]:
                    flat[off : off + p.numel()].copy_(p.data.view(-1))
                    off += p.numel()
            src = dist.get_global_rank(self.process_group, r) if self.process_group else r
            handles.append((r, dist.broadcast(flat, src=src, group=self.process_group,
                                              async_op=True)))
        for r, h in handles:
            h.wait()
            if r == self.rank:
                continue
            off = 0
            for p in self._rank_params[r]:
                p.data.view(-1).copy_(self._flat[r][off : off + p.numel()])
                off += p.numel()

    # -- checkpointing ------------------------------------------------------
    def consolidate_state_dict(self, to=0):
        """Gather all shard optimizer states to rank `to` (C9)."""
        local = {}
        for p in self.shard_params:
            st = self.optim.state.get(p, {})
            idx = self._param_index[id(p)]
            local[idx] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
        if not _dist_active():
            self._consolidated = [local]
            return
        gathered = [None] * self.world_size if self.rank == to else None
        dist.gather_object(local, gathered, dst=to, group=self.process_group)
        if self.rank == to:
            self._consolidated = gathered

    def state_dict(self):
        """torch-format state dict over ALL params (rank 0, post-consolidation)."""
        merged = {}
        if self._consolidated is not None:
            for d in self._consolidated:
                merged.update(d)
        else:
            for p in self.shard_params:
                idx = self._param_index[id(p)]
                st = self.optim.state.get(p, {})
                merged[idx] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
        group = dict(self.optim.param_groups[0])
        group["params"] = list(range(len(self.all_params)))
        return {"state": merged, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        for k, v in groups[0].items():
            if k != "params":
                self.optim.param_groups[0][k] = v
        for idx, st in state_dict["state"].items():
            idx = int(idx)
            p = self.all_params[idx]
            if self.owner[idx] != self.rank:
                continue
            # moments land in the shard optimizer's moment dtype (fp32 under
            # state_dtype=float32, else the parameter's), as AdamW.load_state_dict
            moment_dtype = self.optim._moment_dtype(p)
            self.optim.state[p] = {
                k: ((v.to(device=p.device, dtype=moment_dtype)
                     if k in ("exp_avg", "exp_avg_sq") else v.to(p.device))
                    if torch.is_tensor(v) else v)
                for k, v in st.items()
            }
