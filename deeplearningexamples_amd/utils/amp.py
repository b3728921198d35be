"""The loss-scale state the mixed-precision train steps share."""
import torch

from .. import functional as F


class GradScalerState:
    """Device-resident loss-scale state (torch.cuda.amp.GradScaler semantics, main.py:497)."""

    def __init__(self, device, enabled=True, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=int(1e9)):
        self.enabled = enabled
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        s = init_scale if enabled else 1.0
        self.scale = torch.full((1,), s, dtype=torch.float32, device=device)
        self.inv_scale = torch.full((1,), 1.0 / s, dtype=torch.float32, device=device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=device)
        self.growth_tracker = torch.zeros(1, dtype=torch.int32, device=device)

    def update(self):
        if self.enabled:
            F.amp_update_scale_(self.scale, self.growth_tracker, self.found_inf, self.inv_scale,
                                self.growth_factor, self.backoff_factor, min(self.growth_interval, 2 ** 31 - 1))
