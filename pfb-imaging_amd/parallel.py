"""Band-parallel runtime: one process per GPU, bands sharded round-robin, RCCL band reduce.

Imaging bands are the reference's parallel axis (one Ray actor per band,
/root/reference/src/pfb_imaging/operators/band_worker.py:217-237; driver-side sums
``residual_mfs = sum_b residual_b / wsum``, core/deconv.py:320-321, core/grid.py:430-446).
Here band ``b`` lives on rank ``b % world_size`` for the whole run; gridding, degridding,
Hessian applies and CG need no communication; only the summed dirty/residual image crosses
xGMI, as one large ``reduce(sum)`` to the root rank.

Two transports sit behind the same methods:
  * ``rccl``  -- ``pfbhip_comm_*`` (RCCL over xGMI) on device buffers: the product path on GPUs;
  * ``host``  -- host arrays through :class:`HostGroup`, a plain TCP star on ``MASTER_ADDR``: the rendezvous that carries
                 RCCL's 128-byte unique id from rank 0 to the other ranks, the scalar agreements between ranks
                 (``min/max/sum_over_ranks``), and -- as a whole transport -- the CPU tests of the sharding / reduce logic
                 (there is no GPU in the authoring container).  The launcher's environment (RANK / WORLD_SIZE /
                 LOCAL_RANK / MASTER_ADDR / MASTER_PORT) is all that is read; no framework is imported.
"""

import ctypes as ct
import os
import socket
import struct
import time

import numpy as np

from . import _lib
from ._lib import DeviceArray, check, lib, ptr


class HostGroup:
    """Host-side process group over plain TCP: rank 0 listens, every other rank connects to it (a star).

    The one primitive is ``allgather_bytes``; broadcast and the small reductions are built on it, summed in rank order on
    every rank, so all ranks hold bit-identical results.  It moves rendezvous data and scalars in the product and whole
    arrays only in CPU tests -- the images of the product path travel over RCCL.

    Port: ``PFBHIP_RDZV_PORT`` if set, else the first of ``MASTER_PORT + 1 .. + 16`` rank 0 can bind (``MASTER_PORT`` itself
    belongs to the launcher's own key-value store when the driver's launcher starts the ranks).  Each connection opens with a token that names the
    job (``MASTER_PORT`` and world size), so a foreign listener on a candidate port is skipped, not talked to."""

    MAGIC = b"PFBHIP1\0"
    SPAN = 16

    def __init__(self, rank, world, addr=None, port=None, timeout=None):
        self.rank, self.world = int(rank), int(world)
        self.addr = addr or os.environ.get("MASTER_ADDR", "127.0.0.1")
        base = int(os.environ.get("MASTER_PORT", "29500")) if port is None else int(port)
        fixed = os.environ.get("PFBHIP_RDZV_PORT") if port is None else str(port)
        self.ports = [int(fixed)] if fixed else [base + 1 + k for k in range(self.SPAN)]
        self.token = self.MAGIC + struct.pack("<qq", base, self.world)
        self.timeout = float(os.environ.get("PFBHIP_RDZV_TIMEOUT", "300")) if timeout is None else float(timeout)
        self.peers = []     # rank 0: sockets of ranks 1.., in rank order
        self.sock = None    # other ranks: the socket to rank 0
        if self.world > 1:
            (self._listen if self.rank == 0 else self._connect)()

    # -- wire helpers --------------------------------------------------------------------------------------------
    @staticmethod
    def _recv(sock, n):
        buf = bytearray(n)
        view, got = memoryview(buf), 0
        while got < n:
            k = sock.recv_into(view[got:], n - got)
            if k == 0:
                raise ConnectionError("HostGroup: peer closed the connection")
            got += k
        return bytes(buf)

    @classmethod
    def _send_msg(cls, sock, payload):
        sock.sendall(struct.pack("<q", len(payload)) + payload)

    @classmethod
    def _recv_msg(cls, sock):
        (n,) = struct.unpack("<q", cls._recv(sock, 8))
        return cls._recv(sock, n)

    def _listen(self):
        srv, err = None, None
        for p in self.ports:
            try:
                srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
                srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                srv.bind(("" if self.addr not in ("127.0.0.1", "localhost") else "127.0.0.1", p))
                break
            except OSError as e:
                srv.close()
                srv, err = None, e
        if srv is None:
            raise RuntimeError(f"HostGroup: rank 0 cannot bind any of the ports {self.ports}: {err}")
        srv.listen(self.world + 8)
        srv.settimeout(1.0)
        deadline = time.time() + self.timeout
        got = {}
        while len(got) < self.world - 1:
            if time.time() > deadline:
                srv.close()
                raise TimeoutError(f"HostGroup: {len(got) + 1} of {self.world} ranks arrived within {self.timeout:.0f} s")
            try:
                c, _ = srv.accept()
            except socket.timeout:
                continue
            try:
                c.settimeout(5.0)
                hello = self._recv(c, len(self.token) + 8)
                (r,) = struct.unpack("<q", hello[len(self.token):])
                if hello[:len(self.token)] != self.token or not 0 < r < self.world or r in got:
                    raise ConnectionError("not ours")
                c.sendall(self.MAGIC)
                c.settimeout(None)
                c.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                got[r] = c
            except (OSError, struct.error):
                c.close()
        srv.close()
        self.peers = [got[r] for r in range(1, self.world)]

    def _connect(self):
        deadline = time.time() + self.timeout
        hello = self.token + struct.pack("<q", self.rank)
        while True:
            for p in self.ports:
                try:
                    s = socket.create_connection((self.addr, p), timeout=3.0)
                except OSError:
                    continue
                try:
                    s.settimeout(4.0)
                    s.sendall(hello)
                    if self._recv(s, len(self.MAGIC)) == self.MAGIC:
                        s.settimeout(None)
                        s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                        self.sock = s
                        return
                except OSError:
                    pass
                s.close()
            if time.time() > deadline:
                raise TimeoutError(f"HostGroup: rank {self.rank} found no rank 0 on {self.addr}:{self.ports} within "
                                   f"{self.timeout:.0f} s")
            time.sleep(0.05)

    # -- collectives ---------------------------------------------------------------------------------------------
    def allgather_bytes(self, payload):
        """Every rank's payload, as a list in rank order, on every rank."""
        payload = bytes(payload)
        if self.world == 1:
            return [payload]
        if self.rank == 0:
            parts = [payload] + [self._recv_msg(c) for c in self.peers]
            blob = b"".join(struct.pack("<q", len(p)) + p for p in parts)
            for c in self.peers:
                self._send_msg(c, blob)
            return parts
        self._send_msg(self.sock, payload)
        blob, parts, off = self._recv_msg(self.sock), [], 0
        for _ in range(self.world):
            (n,) = struct.unpack_from("<q", blob, off)
            parts.append(blob[off + 8:off + 8 + n])
            off += 8 + n
        return parts

    def bcast_bytes(self, payload, src=0):
        return self.allgather_bytes(payload if self.rank == src else b"")[src]

    def allgather(self, arr):
        """float64 blocks of equal shape from every rank, stacked along a new leading axis (rank order)."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        parts = self.allgather_bytes(arr.tobytes())
        return np.stack([np.frombuffer(p, dtype=np.float64).reshape(arr.shape) for p in parts])

    def barrier(self):
        self.allgather_bytes(b"")

    def close(self):
        for c in self.peers + ([self.sock] if self.sock is not None else []):
            try:
                c.close()
            except OSError:
                pass
        self.peers, self.sock = [], None


def band_owner(band, world_size):
    return band % world_size


def local_bands(nband, rank, world_size):
    return [b for b in range(nband) if band_owner(b, world_size) == rank]


_HOST_GROUPS = {}


class BandComm:
    def __init__(self, rank=0, world_size=1, local_rank=0, transport=None, host=None):
        self.rank, self.world_size, self.local_rank = rank, world_size, local_rank
        self.transport = transport
        self._h = None
        self._host = host   # HostGroup (or a test stand-in with the same methods) when world_size > 1

    # -- construction ------------------------------------------------------
    @classmethod
    def from_env(cls, transport=None, set_device=True, host=None):
        """Build from the launcher's environment (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT).

        ``transport``: "rccl" (default on a box with GPUs) or "host" (host arrays over :class:`HostGroup`; CPU tests).
        ``host`` replaces the TCP group by an object with the same methods (the gloo stand-in of the CPU tests)."""
        rank = int(os.environ.get("RANK", "0"))
        world = int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if transport is None:
            transport = "rccl" if _lib.device_count() > 0 else "host"
        if transport not in ("rccl", "host"):
            raise ValueError(f"unknown transport {transport!r} (rccl | host)")
        self = cls(rank, world, local_rank, transport, host)
        if transport == "rccl" and set_device:
            ndev = _lib.device_count()
            check(lib().pfbhip_set_device(local_rank % max(ndev, 1)))
        if world > 1 and self._host is None:
            # one TCP group per process and job: a second communicator (bench.py's fallback when RCCL fails on SOME rank)
            # must not make the ranks rendezvous again -- the ranks that did not fail would not come
            key = (rank, world, os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))
            if key not in _HOST_GROUPS:
                _HOST_GROUPS[key] = HostGroup(rank, world)
            self._host = _HOST_GROUPS[key]
        if transport == "rccl":
            uid = np.zeros(_lib.UNIQUE_ID_BYTES, dtype=np.uint8)
            if rank == 0:
                check(lib().pfbhip_comm_unique_id(ptr(uid)))
            if world > 1:  # RCCL's unique id travels rank 0 -> all over the TCP group
                uid = np.frombuffer(self._host.bcast_bytes(uid.tobytes(), src=0), dtype=np.uint8).copy()
            h = ct.c_void_p()
            check(lib().pfbhip_comm_create(ptr(uid), world, rank, ct.byref(h)))
            self._h = h
        return self

    def close(self):
        if self._h is not None and self._h.value:
            lib().pfbhip_comm_destroy(self._h)
            self._h = None
        self._host = None   # the process-wide TCP group stays up for later communicators (closed at exit)

    # -- collectives ----------------------------------------------------------
    def barrier(self):
        if self.world_size == 1:
            return
        if self.transport == "rccl":
            check(lib().pfbhip_comm_barrier(self._h))
        else:
            self._host.barrier()

    def reduce_sum_dev(self, send, recv, root=0):
        """RCCL sum-to-root of device buffers (the product's band reduce)."""
        assert self.transport == "rccl"
        n = int(np.prod(send.shape, dtype=np.int64))
        # non-root ranks pass their send buffer as the (unused) receive buffer, the usual NCCL idiom
        rptr = send.ptr if recv is None else recv.ptr
        check(lib().pfbhip_comm_reduce_sum(self._h, send.ptr, rptr, n, root))

    def allreduce_sum_dev(self, send, recv):
        assert self.transport == "rccl"
        n = int(np.prod(send.shape, dtype=np.int64))
        check(lib().pfbhip_comm_allreduce_sum(self._h, send.ptr, recv.ptr, n))

    def reduce_sum(self, arr, root=0):
        """Sum a float64 host array over ranks; the root gets the total, others get None."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if self.world_size == 1:
            return arr
        if self.transport == "rccl":  # upload -> ncclReduce -> download on the communicator's persistent staging buffer
            out = _lib.result_empty(arr.shape, np.float64) if self.rank == root else None
            check(lib().pfbhip_comm_reduce_sum_host(self._h, ptr(arr), ptr(out), arr.size, root))
            return out
        tot = self._host.allgather(arr).sum(axis=0)
        return tot if self.rank == root else None

    def allreduce_sum(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if self.world_size == 1:
            return arr
        if self.transport == "rccl":
            out = arr.copy()
            check(lib().pfbhip_comm_allreduce_sum_host(self._h, ptr(out), out.size))
            return out
        return self._host.allgather(arr).sum(axis=0)

    def allgather(self, arr):
        """Blocks of equal shape from every rank, stacked along a new leading axis (rank order)."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if self.world_size == 1:
            return arr[None]
        if self.transport == "rccl":
            out = _lib.result_empty((self.world_size,) + arr.shape, np.float64)
            check(lib().pfbhip_comm_allgather_host(self._h, ptr(arr), ptr(out), arr.size))
            return out
        return self._host.allgather(arr)

    def _scalars(self, value):
        return self._host.allgather(np.array([float(value)]))[:, 0]

    def max_over_ranks(self, value):
        return float(value) if self.world_size == 1 else float(self._scalars(value).max())

    def min_over_ranks(self, value):
        return float(value) if self.world_size == 1 else float(self._scalars(value).min())

    def sum_over_ranks(self, value):
        return float(value) if self.world_size == 1 else float(self._scalars(value).sum())


def row_block(nrow, rank, world_size):
    """Contiguous block of rows owned by `rank` (sizes differ by at most one)."""
    base, rem = divmod(nrow, world_size)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def partition_rows_by_w(uvw, freq, world_size, plane_cost=1.0, vis_cost=0.0, support=0.125, mask=None):
    """Rows of ONE band dealt to ``world_size`` ranks as contiguous ranges of |w|: ``[rows_of_rank_0, rows_of_rank_1, ...]``
    (index arrays into the caller's row axis, each sorted by |w|).

    A w-stacking plan transforms ``P = (w_max - w_min) / dw + W`` planes for the w range of ITS visibilities (w in
    wavelengths, |w| after the Hermitian fold), whatever their number -- and at BASELINE config 5 (64 planes) the plane
    transforms are three quarters of an apply.  Time-ordered row blocks all span the full w range, so every rank would
    transform all the planes; ranges of |w| give rank r about ``P / N + W`` of them.

    The boundaries minimise the largest per-rank cost, in units of one single-GPU apply:
    ``plane_cost * (span_r / span + support) + vis_cost * nvis_r / nvis`` -- ``span_r`` the range of |w| f over the rank's rows
    and channels, ``support = W / P0`` the kernel support in units of the single plan's plane count (the planes every rank
    pays on top of its share of the span), ``plane_cost`` / ``vis_cost`` the plane-transform and scatter / gather shares of a
    single-GPU apply (0.73 / 0.27 at C5).  Bisection on the maximum with a greedy sweep over the |w|-sorted rows.
    Deterministic: every rank computes the same partition from the same arrays.
    """
    uvw = np.asarray(uvw, dtype=np.float64)
    freq = np.asarray(freq, dtype=np.float64)
    nrow = uvw.shape[0]
    if world_size <= 1 or nrow == 0:
        return [np.arange(nrow)] + [np.arange(0) for _ in range(max(world_size, 1) - 1)]
    wabs = np.abs(uvw[:, 2])
    order = np.argsort(wabs, kind="stable")
    ws = wabs[order]
    nvis_row = np.full(nrow, freq.size, dtype=np.float64) if mask is None else np.asarray(mask, dtype=bool).sum(axis=1)[order].astype(np.float64)
    cum = np.concatenate([[0.0], np.cumsum(nvis_row)])
    tot = max(cum[-1], 1.0)
    fmin, fmax = float(freq.min()), float(freq.max())
    lo_all, hi_all = ws[0] * fmin, ws[-1] * fmax       # span of |w| f over rows x channels (up to the common 1 / c)
    span = max(hi_all - lo_all, 1e-300)
    over = float(support)
    # cost of rows [a, b): plane term from its own span (+ the kernel support), visibility term from its count
    def cost(a, b):
        if b <= a:
            return 0.0
        return plane_cost * ((ws[b - 1] * fmax - ws[a] * fmin) / span + over) + vis_cost * (cum[b] - cum[a]) / tot

    def sweep(limit):
        """Greedy: extend each rank's range while its cost stays <= limit; returns the boundaries or None."""
        bounds, a = [0], 0
        for _ in range(world_size):
            lo, hi = a, nrow                            # largest b with cost(a, b) <= limit (cost is monotone in b)
            if cost(a, min(a + 1, nrow)) > limit and a < nrow:
                return None
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if cost(a, mid) <= limit:
                    lo = mid
                else:
                    hi = mid - 1
            a = lo
            bounds.append(a)
            if a == nrow:
                break
        if bounds[-1] < nrow:
            return None
        bounds += [nrow] * (world_size + 1 - len(bounds))
        return bounds

    lo_c, hi_c = 0.0, cost(0, nrow)
    best = sweep(hi_c)
    for _ in range(50):
        mid = 0.5 * (lo_c + hi_c)
        got = sweep(mid)
        if got is None:
            lo_c = mid
        else:
            best, hi_c = got, mid
    return [order[best[r]:best[r + 1]] for r in range(world_size)]


class RowShardedGridder:
    """ONE band's visibilities split into contiguous row blocks, one block per GPU.

    The sharding for a single very large band (BASELINE config 5: 1e8 visibilities, 64 w-planes,
    8 GPUs): gridding is additive over rows (/root/reference/tests/test_imager_pass2.py:45-63), so
    every rank grids its block into a private image and the images are summed over xGMI
    (``reduce``/``all-reduce``); degridding needs no exchange (every rank holds the image and
    predicts its own rows).  Each rank's plan chooses its own kernel / w-plane layout for the w
    range of its block; every partial result is within epsilon of its own DFT sum.

    ``gridder_cls`` is injectable so the host logic can be tested without a GPU.
    """

    def __init__(self, comm, uvw, freq, mask=None, gridder_cls=None, **kw):
        if gridder_cls is None:
            from .wgridder import Gridder as gridder_cls
        self.comm = comm
        self.nrow = uvw.shape[0]
        self.r0, self.r1 = row_block(self.nrow, comm.rank, comm.world_size)
        sl = self._select()
        self.local = gridder_cls(uvw[sl], freq, None if mask is None else mask[sl], **kw)

    def _select(self):
        """The rows of this rank (a slice here; an index array in WShardedGridder)."""
        return slice(self.r0, self.r1)

    def _rows(self, a):
        return None if a is None else a[self._select()]

    def _device_exchange(self):
        """True when the partial images can stay in HBM between the local gridder and the collective."""
        return self.comm.world_size > 1 and self.comm.transport == "rccl" and hasattr(self.local, "vis2dirty_dev")

    def _img_buffers(self):
        if getattr(self, "_dbuf", None) is None:
            shape = (self.local.nx, self.local.ny)
            self._dbuf = (DeviceArray(shape, np.float64), DeviceArray(shape, np.float64))
        return self._dbuf

    def vis2dirty(self, vis, wgt=None, root=None):
        """Sum over ranks of the partial dirty images: on every rank (``root=None``) or on ``root`` only."""
        if self._device_exchange():  # partial image -> xGMI sum -> ONE download, on persistent device buffers
            part, _ = self._img_buffers()
            self.local.vis2dirty_dev(self._rows(vis), self._rows(wgt), part)
            if root is None:
                self.comm.allreduce_sum_dev(part, part)
                return part.download()
            self.comm.reduce_sum_dev(part, part if self.comm.rank == root else None, root=root)
            return part.download() if self.comm.rank == root else None
        part = self.local.vis2dirty(self._rows(vis), self._rows(wgt))
        if root is None:
            return self.comm.allreduce_sum(part).reshape(part.shape)
        out = self.comm.reduce_sum(part, root=root)
        return None if out is None else out.reshape(part.shape)

    def dirty2vis(self, dirty, wgt=None):
        """Model visibilities of THIS rank's rows, shape (r1 - r0, nchan); no communication."""
        return self.local.dirty2vis(dirty, self._rows(wgt))

    def set_weights(self, wgt):
        self.local.set_weights(self._rows(wgt))

    def hessian(self, x, beam=None, eta=0.0, wsum=0.0):
        """beam R^H W R (beam x) / wsum + eta x over ALL rows: local partials + one all-reduce."""
        if self._device_exchange():
            xd, od = self._img_buffers()
            xd.upload(x)
            bd = None
            if beam is not None:
                bd = DeviceArray.from_host(np.ascontiguousarray(beam, dtype=np.float64))
            self.local.hessian_dev(xd, od, beam_dev=bd, eta=0.0, wsum=wsum)
            self.comm.allreduce_sum_dev(od, od)
            out = od.download()
            if bd is not None:
                bd.free()
        else:
            part = self.local.hessian(x, beam=beam, eta=0.0, wsum=wsum)
            out = self.comm.allreduce_sum(part).reshape(part.shape)
        if eta:
            out = out + eta * x
        return out

    def close(self):
        for d in getattr(self, "_dbuf", None) or ():
            d.free()
        self._dbuf = None
        self.local.close()


class WShardedGridder(RowShardedGridder):
    """ONE band's visibilities split by |w|: rank r owns a contiguous range of |w| (see :func:`partition_rows_by_w`), hence
    only the w-planes of that range -- the split of SURVEY.md section 8(e) ("shard w-planes") for a single very large band
    (BASELINE config 5: 1e8 visibilities, 64 w-planes, 8 GPUs).  Everything else is :class:`RowShardedGridder`: gridding is
    additive over rows (/root/reference/tests/test_imager_pass2.py:45-63), so the partial images are summed with one
    ``reduce`` / ``all-reduce`` over xGMI; degridding needs the image on every rank (the caller's broadcast) and no exchange;
    ``dirty2vis`` returns the model visibilities of ``self.rows`` (this rank's rows, in |w| order).

    ``plane_share`` is the plane-transform share of a single-GPU apply (0.73 at C5, ``profiles/r02f_bench_C5.json``); the
    rest is attributed to the scatter / gather, which scales with the visibility count.
    """

    def __init__(self, comm, uvw, freq, mask=None, gridder_cls=None, plane_share=0.73, support_planes=8, planes_estimate=64, **kw):
        self.parts = partition_rows_by_w(uvw, freq, comm.world_size, plane_cost=plane_share, vis_cost=1.0 - plane_share,
                                         support=support_planes / max(planes_estimate, 1), mask=mask)
        self.rows = self.parts[comm.rank] if comm.world_size > 1 else np.arange(uvw.shape[0])
        super().__init__(comm, uvw, freq, mask, gridder_cls=gridder_cls, **kw)

    def _select(self):
        return self.rows if self.comm.world_size > 1 else slice(None)   # (one rank: every row, in the caller's order, no copy)

    def planes_per_rank(self):
        """w-planes of every rank's plan (0 for a stand-in gridder without ``info``), gathered over the communicator."""
        mine = float(getattr(self.local, "info", {}).get("nplanes", 0)) if hasattr(self.local, "info") else 0.0
        if self.comm.world_size == 1:
            return [int(mine)]
        v = np.zeros(self.comm.world_size)
        v[self.comm.rank] = mine
        return [int(p) for p in self.comm.allreduce_sum(v)]
