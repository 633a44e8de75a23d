"""nerf.OccupancyGrid: a bit per cell of a box in the network's input space - set where the density field may exceed a level - that
nerf.render_dex_depth(occupancy=...) uses to evaluate the density networks only on the ray samples that fall into set cells
(include/dexnerf_hip_occupancy.h has the definition of the bits and of a sample's cell), and nerf.LiveOccupancyGrid: such a grid kept
up to date on the device beside networks that are still training (include/dexnerf_hip_live.h)."""
import numpy as np
import torch

from . import _hip, _ops
from .train_utils import _density_pack, density_grid


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


class LiveOccupancyGrid:
    """An occupancy grid that lives beside networks while they train (include/dexnerf_hip_live.h has the definition): `ema`, one fp32
    per cell, is a decayed running maximum of the raw density the networks give at one jittered point of the cell per refresh, and the
    cell's bit is set while that exceeds `level` (strict, fp32: the Dex comparison) or the density there was not finite, dilated by
    `dilate` cells.  nerf.FusedTrainStep(ray_span=live) refreshes it every occupancy_update_every iterations and tightens every training
    ray's near / far to its occupied span (OccupancyGrid.ray_spans).

    The bits start ALL SET and the first `warmup_updates` refreshes only feed `ema`: until then the grid tightens nothing.  `bits` is
    allocated once and only ever written in place, so a captured HIP graph that reads it sees every refresh.  The points are drawn from
    the grid's own rng record (seed, refreshes so far) - not the training step's -, so every rank of a data-parallel run refreshes the
    same bits from the same weights, and a grid resumed from state_dict() continues with the same draws.

    What it does not promise: one point per cell and refresh is a sample, and the networks' density early in training is not the
    scene's - a level or a warm-up that is too eager clears cells the scene occupies, and rays through them then get no samples there
    (a missed ray keeps its whole [near, far])."""

    def __init__(self, bounds, cells, device, level=0.01, decay=0.95, dilate=1, warmup_updates=4, seed=0):
        b, c, _ = _ops.check_occupancy_grid(bounds, cells, "LiveOccupancyGrid")
        self.level, self.decay, self.dilate = _ops.check_live_occupancy(level, decay, dilate, "LiveOccupancyGrid")
        self.sizes = _ops.occupancy_cell_sizes(b, c)
        self.warmup_updates, self.seed = int(warmup_updates), int(seed)
        if self.warmup_updates < 0:
            raise ValueError(f"LiveOccupancyGrid: warmup_updates must be >= 0, got {warmup_updates}")
        device = torch.device(device)
        n = c[0] * c[1] * c[2]
        n_words = _ops.occupancy_words(c)
        words = np.full(n_words, 0xFFFFFFFF, np.uint32)
        if n % 32:
            words[-1] = (1 << (n % 32)) - 1          # the bits past the last cell are 0, as in every grid
        self._grid = OccupancyGrid(torch.from_numpy(words.view(np.int32).copy()).to(device), b, c)
        self.ema = torch.zeros(n, dtype=torch.float32, device=device)
        self.scratch = torch.zeros(n_words, dtype=torch.int32, device=device) if self.dilate > 0 else None
        self.rng_state = _ops.new_rng_state(self.seed, device)
        self.updates_done = 0                         # host side: refreshes so far

    @property
    def grid(self):
        """The OccupancyGrid of the bits - the same object and the same tensor for the life of this grid."""
        return self._grid

    @property
    def bits(self):
        return self._grid.bits

    @property
    def bounds(self):
        return self._grid.bounds

    @property
    def cells(self):
        return self._grid.cells

    @property
    def device(self):
        return self._grid.bits.device

    def update(self, models, encode_position_fn, max_points=1 << 22):
        """One refresh: the cell points (dn_occupancy_cell_points, in slabs of at most max_points cells), the raw density of each
        model's density pack on them (_ops.run_network_pts: no-grad, nerf.set_precision's 'fp32' or bf16, 'fp16' raises - density_grid's
        guards), and dn_occupancy_ema_update, which writes the bits once `warmup_updates` refreshes have gone before.  No host read;
        ordinary launches on the current stream - legal between two replays of a captured step, not inside a capture of one that
        is to refresh more than once (the warm-up is counted on the host)."""
        models = [m for m in (models if isinstance(models, (list, tuple)) else [models]) if m is not None]
        if not 1 <= len(models) <= 2:
            raise ValueError(f"LiveOccupancyGrid.update: one or two density networks, got {len(models)}")
        max_points = int(max_points)
        if max_points < 1:
            raise ValueError("LiveOccupancyGrid.update: max_points must be at least 1")
        with torch.no_grad():
            packs = [_density_pack(m, encode_position_fn, "LiveOccupancyGrid.update") for m in models]
        dev = self.device
        if not dev.type == "cuda":
            raise RuntimeError("LiveOccupancyGrid.update: runs on the ROCm device only (the grid lives on the host); build it with device='cuda'")
        for m in models:
            if m.layer1.weight.device != dev:
                raise ValueError(f"LiveOccupancyGrid.update: the grid lives on {dev} and a network on {m.layer1.weight.device}")
        g = self._grid
        n = self.ema.numel()
        with torch.no_grad():
            if n <= max_points:
                pts = _ops.occupancy_cell_points(g.bounds, g.cells, self.sizes, 0, n, self.rng_state)
                columns = [_ops.run_network_pts(pack, pts, None, 1)[:, 3] for pack in packs]
            else:
                sigma = torch.empty((len(packs), n), dtype=torch.float32, device=dev)
                for c0 in range(0, n, max_points):
                    count = min(max_points, n - c0)
                    pts = _ops.occupancy_cell_points(g.bounds, g.cells, self.sizes, c0, count, self.rng_state)
                    for q, pack in enumerate(packs):
                        sigma[q, c0:c0 + count] = _ops.run_network_pts(pack, pts, None, 1)[:, 3]
                columns = [sigma[q] for q in range(len(packs))]
            _ops.occupancy_ema_update(columns, g.cells, self.decay, self.level, self.updates_done >= self.warmup_updates, self.dilate,
                                      self.ema, g.bits, self.scratch, self.rng_state)
        self.updates_done += 1

    def occupied_fraction(self):
        """Set cells / cells (a host read)."""
        return self._grid.occupied_fraction()

    def state_dict(self):
        """ema, bits, bounds, cells, the settings, the rng record and the refresh counter, on the host."""
        return dict(ema=self.ema.detach().cpu(), bits=self._grid.bits.detach().cpu(), bounds=tuple(self.bounds), cells=tuple(self.cells),
                    level=self.level, decay=self.decay, dilate=self.dilate, warmup_updates=self.warmup_updates, seed=self.seed,
                    rng_state=self.rng_state.detach().cpu(), updates_done=int(self.updates_done))

    @classmethod
    def from_state_dict(cls, state, device=None):
        """The grid `state` was taken from: the next update() draws what the original's next update() draws."""
        ema = torch.as_tensor(state["ema"], dtype=torch.float32)
        live = cls(state["bounds"], state["cells"], ema.device if device is None else device, level=state["level"], decay=state["decay"],
                   dilate=state["dilate"], warmup_updates=state["warmup_updates"], seed=state["seed"])
        bits, rng = torch.as_tensor(state["bits"], dtype=torch.int32), torch.as_tensor(state["rng_state"], dtype=torch.int32)
        if ema.shape != live.ema.shape or bits.shape != live.bits.shape or rng.shape != live.rng_state.shape:
            raise ValueError(f"LiveOccupancyGrid.from_state_dict: ema, bits and the rng record do not fit cells {live.cells}")
        live.ema.copy_(ema); live.bits.copy_(bits); live.rng_state.copy_(rng)
        live.updates_done = int(state["updates_done"])
        if live.updates_done < 0:
            raise ValueError("LiveOccupancyGrid.from_state_dict: a negative refresh counter")
        return live
