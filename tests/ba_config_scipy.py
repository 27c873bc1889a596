"""tests/ba_scipy.py's independent solver with a point mask, for the accuracy check of tests/test_ba_config_cpu.py
(DESIGN.md 15.12): a constant point stays at its start and has no unknowns; everything else is ba_scipy's."""
from __future__ import annotations

import numpy as np

import ba_scipy


class MaskedProblem(ba_scipy.Problem):
    def __init__(self, *args, point_const, **kw):
        super().__init__(*args, **kw)
        self.xvar = np.flatnonzero(np.asarray(point_const).reshape(-1) == 0)
        self.nhead = self.n - self.X0.size
        self.n = self.nhead + 3 * self.xvar.size

    def unpack(self, x):
        dX = np.zeros_like(self.X0)
        dX[self.xvar] = x[self.nhead:].reshape(-1, 3)
        return super().unpack(np.concatenate([x[:self.nhead], dX.reshape(-1)]))
