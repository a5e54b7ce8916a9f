"""MISE on the device (csrc/giga_mise.hip through giga_mise_*): the sparse value grid of the reference's `generate_from_latent`
(conv_onet/generation.py:125-142, utils/libmise/mise.pyx).  `MISE` keeps the state of B independent octrees in one device
workspace and is driven like libmise's class -- `query()`, `update(values)`, `to_dense()` -- with device tensors in place of numpy
arrays; `mise_grid` is the loop of generation.py:128-141.  Per round the only device-to-host traffic is the B counts."""
import numpy as np
import torch

from . import _capi


def lin_table(resolution, box_size):
    """float32 [resolution + 1]: `box_size * (i / resolution - 0.5)` evaluated in float64 and rounded once, the coordinate of lattice
    index i as generation.py:132-135 computes it (`points / mesh_extractor.resolution`, `box_size * (pointsf - 0.5)` in float64,
    float32 when the points reach the network)."""
    i = np.arange(int(resolution) + 1, dtype=np.float64)
    return (float(box_size) * (i / float(resolution) - 0.5)).astype(np.float32)


class MISE:
    """MISE(resolution0, depth, threshold) of libmise for `batch` scenes at once.  `resolution` = resolution0 << depth; a point is
    its linear index (i * N + j) * N + k on the N = resolution + 1 lattice."""

    def __init__(self, resolution0, depth, threshold, batch=1, device=None, lin=None):
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise _capi.GigaHipError("MISE runs only on a HIP device (got %s); there is no CPU fallback" % dev)
        self.resolution0, self.depth, self.threshold, self.batch = int(resolution0), int(depth), float(threshold), int(batch)
        self.resolution = self.resolution0 << max(self.depth, 0)
        self.n = self.resolution + 1
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        L = _capi.lib()
        nbytes = L.giga_mise_workspace_bytes(self.batch, self.resolution0, self.depth)
        if nbytes == 0:
            raise _capi.GigaHipError(f"MISE(resolution0={resolution0}, depth={depth}, batch={batch}) is outside the supported range "
                                     f"(resolution0 >= 1, depth >= 1, at most {_capi.MISE_MAX_N} samples per axis, batch >= 1)")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._lin = None
        if lin is not None:
            lin = torch.as_tensor(lin, dtype=torch.float32)
            if tuple(lin.shape) != (self.n,):
                raise ValueError(f"expected a per-axis table of {self.n} coordinates, got {tuple(lin.shape)}")
            self._lin = lin.to(self.device).contiguous()
        self._counts_dev = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._query = None
        self.counts = None                 # host list of the last query's lengths
        self.points = None                 # (B, L, 3) coordinates of the last query (with a `lin` table)
        _capi.call("giga_mise_init", self.device, *self._shape(), self._ws, self._ws.numel())

    def _shape(self):
        return self.batch, self.resolution0, self.depth

    def query(self):
        """The unknown points of every scene: (B, L) int32 linear indices on the device, ascending inside a scene, L = the longest
        list; `self.counts` (host) holds the B lengths, and entries past a scene's length are 0 (a valid index).  With a `lin` table
        `self.points` (B, L, 3) holds the coordinates, padded with a repeated valid point."""
        _capi.call("giga_mise_count", self.device, *self._shape(), self._ws, self._ws.numel(), self._counts_dev)
        self.counts = self._counts_dev.cpu().tolist()
        cap = max(self.counts)
        self._query = torch.zeros((self.batch, cap), dtype=torch.int32, device=self.device)
        self.points = torch.empty((self.batch, cap, 3), dtype=torch.float32, device=self.device) if self._lin is not None else None
        _capi.call("giga_mise_emit", self.device, *self._shape(), self._ws, self._ws.numel(), self._query, cap, None, self._lin,
                   self.points)
        return self._query

    def update(self, values):
        """values (B, L) float32 on the device, column i of scene b the value at `query()[b, i]` (columns past the scene's length are
        ignored): mark them known, subdivide every leaf that sees both sides of the threshold."""
        if self._query is None:
            raise _capi.GigaHipError("MISE.update needs the list of a preceding query()")
        _capi.require_device(values)
        if tuple(values.shape) != tuple(self._query.shape):
            raise ValueError(f"expected values of shape {tuple(self._query.shape)}, got {tuple(values.shape)}")
        v = values.detach().to(self.device, torch.float32).contiguous()
        _capi.call("giga_mise_update", self.device, v, self._query, self._query.shape[1], *self._shape(), self.threshold, self._ws,
                   self._ws.numel())
        self._query = None

    def to_dense(self):
        """(B, N, N, N) float32 on the device (mise.pyx:130-164)."""
        out = torch.empty((self.batch, self.n, self.n, self.n), dtype=torch.float32, device=self.device)
        _capi.call("giga_mise_to_dense", self.device, *self._shape(), self._ws, self._ws.numel(), out)
        return out


def mise_grid(value_fn, resolution0, depth, threshold, batch=1, device=None, lin=None, stats=None, rounds=None):
    """generation.py:128-141: query, evaluate, update until every scene's query is empty; returns the (B,N,N,N) dense grid.
    `value_fn(query, points)` gets the (B, L) indices and the (B, L, 3) coordinates (None without `lin`) and returns (B, L) values,
    all on the device.  `stats` (dict) receives "mise rounds" and "mise points" (evaluated samples of all scenes, padding not
    counted); `rounds` (list) the per-round (query, counts) for tests."""
    m = MISE(resolution0, depth, threshold, batch=batch, device=device, lin=lin)
    n_rounds = n_points = 0
    q = m.query()
    while q.shape[1] != 0:
        if rounds is not None:
            rounds.append((q, list(m.counts)))
        n_rounds, n_points = n_rounds + 1, n_points + sum(m.counts)
        m.update(value_fn(q, m.points))
        q = m.query()
    if stats is not None:
        stats["mise rounds"], stats["mise points"] = n_rounds, n_points
    return m.to_dense()
