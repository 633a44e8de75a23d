"""nerf.OccupancyGrid: a bit per cell of a box in the network's input space - set where the density field may exceed a level - that
nerf.render_dex_depth(occupancy=...) uses to evaluate the density networks only on the ray samples that fall into set cells
(include/dexnerf_hip_occupancy.h has the definition of the bits and of a sample's cell)."""
import numpy as np
import torch

from . import _hip, _ops
from .train_utils import density_grid


class OccupancyGrid:
    """cells (cx,cy,cz) over bounds (x0,y0,z0,x1,y1,z1); cell (i,j,k) has the linear index c = (i*cy + j)*cz + k and is bit c & 31 of
    word c >> 5 of `bits` (int32 words holding the uint32 patterns).  The grid lives in the network's input space: world space, or NDC
    space for forward-facing scenes (dataset.no_ndc False) - nothing converts it.

    It is a sampled approximation: from_networks sets a cell when the density at one of its 8 corners exceeds the level, and the
    density can exceed it between corners; `dilate` sets the neighbours of every such cell too.  eval_nerf.py --occupancy-check reports
    what a grid costs in Dex depths on a scene."""

    def __init__(self, bits, bounds, cells):
        self.bounds, self.cells, self.scale = _ops.check_occupancy_grid(bounds, cells, "OccupancyGrid")
        if not (torch.is_tensor(bits) and bits.dtype == torch.int32 and bits.dim() == 1 and bits.numel() == _ops.occupancy_words(self.cells)):
            raise ValueError(f"OccupancyGrid: bits must be a 1-D int32 tensor of {_ops.occupancy_words(self.cells)} words for cells {self.cells}")
        self.bits = bits.contiguous()

    @property
    def device(self):
        return self.bits.device

    def to(self, device):
        return OccupancyGrid(self.bits.to(device), self.bounds, self.cells)

    @classmethod
    def from_networks(cls, models, encode_position_fn, bounds, cells, level=0.0, dilate=1, max_points=1 << 24):
        """The grid of one or more density networks (coarse and fine: both passes of the render are culled by the same grid, so it must
        cover both): for each model, density_grid at resolution cells + 1 samples the raw density at the cells' corners, and
        dn_occupancy_build sets a cell iff a corner is non-finite or > level (strict, fp32: the Dex comparison), dilated by `dilate`
        cells; the second model on is OR-ed into the same bits.  Guards and precision are density_grid's: no-grad, device networks the
        fused kernels cover, nerf.set_precision's 'fp32' or bf16, 'fp16' raises.  Every argument is judged before any GPU work."""
        models = [m for m in (models if isinstance(models, (list, tuple)) else [models]) if m is not None]
        if not models:
            raise ValueError("OccupancyGrid.from_networks: needs at least one model")
        b, c, _ = _ops.check_occupancy_grid(bounds, cells, "OccupancyGrid.from_networks")
        level, dilate = float(level), int(dilate)
        if not (np.isfinite(level) and abs(level) <= float(np.finfo(np.float32).max)):
            raise ValueError(f"OccupancyGrid.from_networks: level must be finite as fp32, got {level!r}")
        if not 0 <= dilate <= _hip.OCC_MAX_DILATE:
            raise ValueError(f"OccupancyGrid.from_networks: dilate must be 0 .. {_hip.OCC_MAX_DILATE}, got {dilate}")
        bits = None
        for m in models:
            field = density_grid(m, encode_position_fn, b, tuple(n + 1 for n in c), max_points=max_points)[0]
            bits = _ops.occupancy_build(field, c, level, dilate, bits=bits, accumulate=bits is not None)
        return cls(bits, b, c)

    @classmethod
    def from_mask(cls, mask, bounds):
        """The grid whose cell (i,j,k) is set iff mask[i,j,k]: a bool (cx,cy,cz) tensor, packed on the host; the bits live on the mask's
        device."""
        if not (torch.is_tensor(mask) and mask.dtype == torch.bool and mask.dim() == 3 and mask.numel() > 0):
            raise ValueError("OccupancyGrid.from_mask: mask must be a bool (cx, cy, cz) tensor with at least one cell per axis")
        cells = tuple(mask.shape)
        b, c, _ = _ops.check_occupancy_grid(bounds, cells, "OccupancyGrid.from_mask")
        flat = mask.detach().cpu().numpy().reshape(-1)
        packed = np.zeros(4 * _ops.occupancy_words(c), np.uint8)
        by = np.packbits(flat, bitorder="little")
        packed[:by.size] = by
        return cls(torch.from_numpy(packed.view("<u4").astype(np.uint32).view(np.int32).copy()).to(mask.device), b, c)

    def to_mask(self):
        """The bool (cx,cy,cz) tensor of the bits, on their device (unpacked on the host)."""
        words = self.bits.detach().cpu().numpy().view(np.uint32).astype("<u4")
        n = self.cells[0] * self.cells[1] * self.cells[2]
        flat = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        return torch.from_numpy(flat.reshape(self.cells)).to(self.bits.device)

    def occupied_fraction(self):
        """Set cells / cells (a host read)."""
        return float(self.to_mask().float().mean().item())

    def state_dict(self):
        return dict(bits=self.bits.detach().cpu(), bounds=tuple(self.bounds), cells=tuple(self.cells))

    @classmethod
    def from_state_dict(cls, state, device=None):
        bits = torch.as_tensor(state["bits"], dtype=torch.int32)
        return cls(bits if device is None else bits.to(device), state["bounds"], state["cells"])

    def ray_spans(self, rays, pad_cells=1.0, apply=False):
        """(span (N,2), visits (N) int32) of the ray rows (N, >= 8: origin, direction, near, far) - include/dexnerf_hip_span.h: each
        ray walks the grid cell by cell; span is the depth range from the entry of the first set cell to the exit of the last one,
        widened by pad_cells cells of travel and clipped to the row's [near, far]; visits counts the set cells on the way.  A ray that
        meets no set cell is a miss: it keeps its (near, far) and visits 0.  apply=True also writes the span into columns 6 and 7 of
        the hit rows, in place.  nerf.render_dex_depth(ray_span=grid) does exactly that before it renders.

        What the span does not promise: a ray that grazes a cell boundary within fp32 rounding can lose samples the culling
        classification would keep - the pad and the grid's `dilate` are the margins for that; and the grid is a sampled approximation
        of the field."""
        return _ops.occupancy_ray_spans(rays, self, pad_cells, apply)

    def check_render(self, device, who):
        """The refusals of a render with this grid, before any GPU work."""
        if self.bits.device != device:
            raise ValueError(f"{who}: the occupancy grid lives on {self.bits.device} and the rays on {device}; move it with grid.to(device)")
