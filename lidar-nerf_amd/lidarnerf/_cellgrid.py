"""What raycast.py and knn.py share about the uniform cell grid of csrc/cell_grid.h: the limit per axis, the device a build
lands on, the check of a grid_resolution argument and the start of both default-resolution rules."""
import numpy as np
import torch

MAX_CELLS_PER_AXIS = 1024  # kCellMaxPerAxis


def device():
    if not torch.cuda.is_available():
        raise RuntimeError("lidarnerf.raycast: the scene lives on the GPU and none is available (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def grid_triple(grid_resolution, who):
    """An int or three ints as (nx, ny, nz); `who` is the class the error names."""
    is_int = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    g = grid_resolution
    if is_int(g):
        g = (g,) * 3
    else:
        try:
            g = tuple(g)
        except TypeError:
            g = ()
    if len(g) != 3 or not all(is_int(x) for x in g):
        raise ValueError(f"{who}: grid_resolution must be None, an int or three ints, got {grid_resolution!r}")
    g = tuple(int(x) for x in g)
    if any(x < 1 or x > MAX_CELLS_PER_AXIS for x in g):
        raise ValueError(f"{who}: grid_resolution {g}: 1 ... {MAX_CELLS_PER_AXIS} cells per axis")
    return g


def cubic_cells(box, cells):
    """(lo, hi, ext, side) in float64 for `cells` cubic cells over the box (lo[3], hi[3]): ext is the extent per axis with the
    kernel's floor for a flat axis (largest extent / 1024), side the edge of a cube whose volume is the box's / cells."""
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:6], np.float64)
    ext = hi - lo
    emax = float(ext.max()) if float(ext.max()) > 0 else 1.0
    ext = np.maximum(ext, emax / 1024.0)
    side = (float(np.prod(ext)) / max(1.0, float(cells))) ** (1.0 / 3.0)
    return lo, hi, ext, side
