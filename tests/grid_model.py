"""Host model of the device's search grid (csrc/grid.hip: make_grid_meta; csrc/common.h: ball_cells, row_cells, ball_for_each).

For a cloud, a keypoint, a radius and a requested cell it tells which paths of the flattened ball traversal a wave would take:
how many cell rows the ball covers, how many candidates each batch of 64 rows holds and how long the longest single row is. The
tests use it to PROVE, without a GPU, that their scenes reach the second row batch, the second candidate window and a row that
spans windows. The arithmetic is float32 like the device's, but numpy rounds some expressions differently, so the figures are
approximate in the last candidate or two: callers assert with a margin.

The kernel constants are read from the sources, so that a retune makes the path tests fail instead of silently hollowing them."""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-donkey_amd", "csrc")
f32 = np.float32


def _source(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(text, pattern, what):
    m = re.search(pattern, text, re.M)
    assert m, f"{what}: pattern {pattern!r} no longer matches the source"
    return m.group(1)


def constants():
    common, lrf, grid = _source("common.h"), _source("lrf.hip"), _source("grid.hip")
    return dict(
        ROWS_CAP=int(_const(common, r"^#define\s+ISM_ROWS_CAP\s+(\d+)", "ISM_ROWS_CAP")),
        GRID_MAXDIM=int(_const(common, r"^#define\s+ISM_GRID_MAXDIM\s+(\d+)", "ISM_GRID_MAXDIM")),
        GRID_XFRAC=int(_const(common, r"^#define\s+ISM_GRID_XFRAC\s+(\d+)", "ISM_GRID_XFRAC")),
        ROW_BATCH=int(_const(common, r"for \(int r0 = 0; r0 < nrows; r0 \+= (\d+)\)", "rows per batch of ball_for_each")),
        TIE_LDS_KEYS=int(_const(lrf, r"^#define\s+TIE_LDS_KEYS\s+(\d+)", "TIE_LDS_KEYS")),
        TIE_REG_KEYS=int(_const(lrf, r"^#define\s+TIE_REG_KEYS\s+(\d+)", "TIE_REG_KEYS")),
        TIE_BLOCKS=int(_const(lrf, r"const int tie_blocks = (\d+);", "tie workgroups")),
        GRID_FUSED_MAX_PTS=int(_const(grid, r"^#define\s+GRID_FUSED_MAX_PTS\s+(\d+)u", "GRID_FUSED_MAX_PTS")),
        QUEUE=int(_const(_source("shot.hip"), r"float4 qd\[4\]\[(\d+)\]", "SHOT neighbour queue")),
    )


K = constants()


class Grid:
    """GridMeta + cell_start of one object (make_grid_meta and the counting sort that follows it)"""

    def __init__(self, pts, req_cell, xfrac=None):
        pts = np.asarray(pts, f32).reshape(-1, 3)
        pts = pts[np.isfinite(pts).all(1)]
        self.n = len(pts)
        maxdim = K["GRID_MAXDIM"]
        x_frac = f32(1.0) / f32(K["GRID_XFRAC"] if not xfrac else xfrac)
        lo = pts.min(0) if self.n else np.zeros(3, f32)
        hi = pts.max(0) if self.n else np.zeros(3, f32)
        self.minv = lo.astype(f32)
        self.cell = np.zeros(3, f32); self.inv = np.zeros(3, f32); self.dim = np.zeros(3, np.int64)
        for a in range(3):
            cell = f32(req_cell) if req_cell > 0 else f32(1)
            if a == 0:
                cell = f32(cell * x_frac)
            ext = f32(hi[a] - lo[a])
            if not (f32(ext / cell) < f32(maxdim - 1)):
                cell = max(cell, f32(ext / f32(maxdim - 1.5)))
            self.cell[a] = cell
            self.inv[a] = f32(1.0) / cell
            d = int(np.floor(f32(ext * self.inv[a]))) + 1
            self.dim[a] = min(max(d, 1), maxdim)
        if self.n:
            c = np.floor((pts - self.minv) * self.inv).astype(np.int64)
            c = np.clip(c, 0, self.dim - 1)
            cid = (c[:, 2] * self.dim[1] + c[:, 1]) * self.dim[0] + c[:, 0]
            counts = np.bincount(cid, minlength=int(self.dim.prod()))
        else:
            counts = np.zeros(int(self.dim.prod()), np.int64)
        self.cell_start = np.concatenate([[0], np.cumsum(counts)])

    def ball_cells(self, q, r):
        q = np.asarray(q, f32); r = f32(r)
        lo, hi = [0] * 3, [0] * 3
        for a in range(3):
            pad = f32(f32(r * f32(1e-5)) + f32(abs(q[a]) * f32(4e-7))) + f32(1e-30)
            l = int(np.floor(f32(f32(f32(f32(q[a] - r) - pad) - self.minv[a]) * self.inv[a])))
            h = int(np.floor(f32(f32(f32(f32(q[a] + r) + pad) - self.minv[a]) * self.inv[a])))
            if h < 0 or l > self.dim[a] - 1:
                return None
            lo[a] = max(l, 0); hi[a] = min(h, int(self.dim[a]) - 1)
        return lo, hi

    def row_cells(self, cr, gy, gz, q, r):
        lo, hi = cr
        q = np.asarray(q, f32); r = f32(r)
        pad = f32(f32(r * f32(2e-5)) + f32(f32(f32(abs(q[0]) + abs(q[1])) + abs(q[2])) * f32(1e-6))) + f32(1e-30)
        y0 = f32(self.minv[1] + f32(f32(gy) * self.cell[1])); z0 = f32(self.minv[2] + f32(f32(gz) * self.cell[2]))
        dy = max(f32(max(f32(y0 - q[1]), f32(q[1] - f32(y0 + self.cell[1]))) - pad), f32(0))
        dz = max(f32(max(f32(z0 - q[2]), f32(q[2] - f32(z0 + self.cell[2]))) - pad), f32(0))
        rr = f32(r + pad)
        rem = f32(f32(rr * rr) - f32(f32(dy * dy) + f32(dz * dz)))
        if not rem > 0:
            return None
        hc = f32(np.sqrt(rem) + pad)
        l = int(np.floor(f32(f32(f32(q[0] - hc) - self.minv[0]) * self.inv[0])))
        h = int(np.floor(f32(f32(f32(q[0] + hc) - self.minv[0]) * self.inv[0])))
        l = max(l, lo[0]); h = min(h, hi[0])
        return (l, h) if l <= h else None

    def sweep(self, q, r):
        """what ball_for_each does for the ball (q, r): dict(rows, batches = candidates per batch of 64 rows, longest_row, candidates)"""
        cr = self.ball_cells(q, r) if np.isfinite(np.asarray(q, f32)).all() else None
        if cr is None:
            return dict(rows=0, batches=[], longest_row=0, candidates=0)
        lo, hi = cr
        ny = hi[1] - lo[1] + 1
        nrows = ny * (hi[2] - lo[2] + 1)
        lens = np.zeros(nrows, np.int64)
        for j in range(nrows):
            gz, gy = lo[2] + j // ny, lo[1] + j % ny
            xr = self.row_cells(cr, gy, gz, q, r)
            if xr is not None:
                rb = (gz * int(self.dim[1]) + gy) * int(self.dim[0])
                lens[j] = self.cell_start[rb + xr[1] + 1] - self.cell_start[rb + xr[0]]
        nb = K["ROW_BATCH"]
        batches = [int(lens[i:i + nb].sum()) for i in range(0, nrows, nb)]
        return dict(rows=nrows, batches=batches, longest_row=int(lens.max()) if nrows else 0, candidates=int(lens.sum()))
