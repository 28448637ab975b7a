"""ValueEstimator -- drop-in for rlgym_ppo/ppo/value_estimator.py:13-36 on librlppo's fused MLP forward.

Layer sizes that carry a ValueBins (LayerSizes(..., value_head=bins)) build the categorical critic: the last layer has bins.n outputs
and every value is the expectation of softmax(logits) over the bin centres (rlppo_value_bins_readout); logits() gives the raw rows."""
import torch

from .. import _native as N
from ..engine import ptr, stream_ptr
from ._mlp import ArenaModule, build_body


class ValueEstimator(ArenaModule):
    def __init__(self, input_shape, layer_sizes, device):
        super().__init__()
        self.value_bins = getattr(layer_sizes, "value_head", None)
        self.model = build_body(input_shape, layer_sizes, 1 if self.value_bins is None else self.value_bins.n, critic=True)
        self._bins_arg = None if self.value_bins is None else self.value_bins.c_arg()
        self._finish(device)

    def _values(self, out):
        """The network's padded output rows [n, ld_out] -> contiguous values [n]: column 0, or the categorical head's readout."""
        if self.value_bins is None:
            return out[:, 0]
        values = torch.empty(out.shape[0], dtype=torch.float32, device=out.device)
        N.check(N.lib().rlppo_value_bins_readout(stream_ptr(), ptr(out), out.shape[1], self._bins_arg, ptr(values), out.shape[0]))
        return values

    @torch.no_grad()
    def forward(self, x):
        """numpy/tensor [n, d] of any float dtype -> device tensor [n, 1] (value_estimator.py:30-36)."""
        rows = self.arena.stage_obs(x)
        out = self.arena.forward(rows)
        return out[:, :1] if self.value_bins is None else self._values(out).view(-1, 1)

    def forward_padded(self, rows):
        """[n, ld] already-padded device rows -> contiguous [n] values (used by Learner.add_new_experience)."""
        return self._values(self.arena.forward(rows))

    @torch.no_grad()
    def logits(self, x):
        """The categorical head's raw rows: numpy/tensor [n, d] -> device tensor [n, bins.n]."""
        if self.value_bins is None:
            raise ValueError("logits: this critic has one output (build it from LayerSizes(..., value_head=ValueBins(...)))")
        return self.arena.forward(self.arena.stage_obs(x))[:, :self.value_bins.n]
