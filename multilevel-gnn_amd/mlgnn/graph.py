"""Graph topology container: CSR by destination + CSR by source (int32, device resident).

The reference keeps graphs as COO ``edge_index [2, E]`` int64 and lets every layer re-derive its
gather/scatter from it (``MessagePassing.propagate``).  Here the topology is sorted once per batch;
all layers (and forward + backward) share it.
"""
import ctypes
import os

import torch

from . import _lib

# rows (in-edges of a node for the forward, out-edges for the backward) longer than this are cut into chunks that
# run as rows of their own and are combined in order (csrc/hub.hip); 0 disables
HUB_CAP = int(os.environ.get("MLGNN_HUB_CAP", "256"))
# SAGE graphs (narrow rows walked by ONE lane group per row, csrc/aggregate_short.h): rows past this many edges -- a
# transcription factor's targets -- are cut into chunks that the wave-per-row kernel takes (csrc/hub.hip), so a lane
# group never walks more than this many edges on its own
SAGE_HUB_CAP = int(os.environ.get("MLGNN_SAGE_HUB_CAP", "64")) if HUB_CAP > 0 else 0
_SHARED_TOPOLOGY = os.environ.get("MLGNN_SHARED_TOPOLOGY", "1") == "1"      # (0: sort every batch's edge list, for A/B runs)


class CSRGraph:
    """``edge_index[0] = src = j``, ``edge_index[1] = dst = i`` (PyG flow source->target).

    by destination:  rowptr [N+1], col [E] = src, eid [E] = COO position   (stable: COO order kept)
    by source:       rowptr_t [N+1], col_t [E] = dst, pos_t [E] = position in the by-destination
                     order, eid_t [E] = COO position
    """

    def __init__(self, edge_index, num_nodes):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("edge_index must be [2, E]")
        N = int(num_nodes)
        E = int(edge_index.shape[1])
        if N >= 2 ** 31 or E >= 2 ** 31:
            raise ValueError("int32 index range exceeded")
        dev = edge_index.device
        self.num_nodes, self.num_edges, self.device = N, E, dev
        if edge_index.is_cuda:
            self._build_device(edge_index)
        else:
            self._build_host(edge_index)
        self._deg = None
        self._scalar_cache = None
        self._table_cache = None
        self._hub = {}
        self._built = None
        if edge_index.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            self._built = (ev, torch.cuda.current_stream(dev))

    # ---- topology cache --------------------------------------------------------------------------------------------
    # The reference's loader hands the SAME gene-gene topology to every sample of a fold
    # (dataloader/multiloader.py:687-691): a training loop that passes the same edge_index tensor again (or, with
    # ``content=True``, an equal one) gets the CSR it built the first time.
    # Contract: a hit is decided by tensor identity / view + the tensor's VERSION counter.  An edge_index buffer refilled
    # behind autograd's back (``.data``, DLPack, an external kernel) keeps its version: call ``CSRGraph.clear_cache()``
    # after such a refill, or hand the model a prebuilt graph (``batch.csr``).  Entries pin their batch's index tensors
    # and CSR arrays (~0.5 GB at BASELINE configs[1]), so the cache is small: MLGNN_CSR_CACHE entries (default 2, 0 = off;
    # a loader that collates a fresh edge_index per step never hits and should set 0 or attach ``batch.csr``).
    # A hit from another stream than the one that built the graph waits on the build's event.
    _CACHE = []                    # [(edge_index, version, num_nodes, content key or None, graph)], most recent first
    CACHE_SIZE = int(os.environ.get("MLGNN_CSR_CACHE", "2"))
    CACHE_STATS = {"hit": 0, "miss": 0}

    @classmethod
    def from_cache(cls, edge_index, num_nodes, content=False):
        """The CSR of ``edge_index`` from a small most-recently-used cache.  A hit is the same tensor (or another view
        of the same elements) at the same version -- no device work, no synchronisation.  ``content=True`` also matches
        a DIFFERENT tensor with equal contents through a 128-bit checksum computed on the device (one pass over the
        index list and one 16-byte read back: a host synchronisation per lookup, still far cheaper than a build); for
        loaders that collate a fresh but identical ``edge_index`` per batch."""
        N = int(num_nodes)
        if cls.CACHE_SIZE <= 0:
            return cls(edge_index, N)
        for k, ent in enumerate(cls._CACHE):
            if ent[2] == N and ent[1] == edge_index._version and _same_view(ent[0], edge_index):
                cls.CACHE_STATS["hit"] += 1
                cls._CACHE.insert(0, cls._CACHE.pop(k))
                return ent[4]._ordered_after_build()
        key = None
        if content:
            key = _content_key(edge_index)
            for k, ent in enumerate(cls._CACHE):
                if ent[2] == N and ent[3] == key and ent[0].shape == edge_index.shape:
                    cls.CACHE_STATS["hit"] += 1
                    cls._CACHE.insert(0, cls._CACHE.pop(k))
                    return ent[4]._ordered_after_build()
        cls.CACHE_STATS["miss"] += 1
        graph = cls(edge_index, N)
        # (the entry holds the tensor: its storage cannot be recycled under the cache)
        cls._CACHE.insert(0, (edge_index, edge_index._version, N, key, graph))
        del cls._CACHE[cls.CACHE_SIZE:]
        return graph

    @classmethod
    def clear_cache(cls):
        del cls._CACHE[:]

    @classmethod
    def replicated(cls, single, copies):
        """``copies`` block-diagonal copies of the device graph ``single`` (``mlgnn_csr_replicate``): bit for bit the CSR
        of the batched edge list a PyG collate makes of ``copies`` samples that share one topology."""
        n, e, B = single.num_nodes, single.num_edges, int(copies)
        if not single.rowptr.is_cuda:
            raise RuntimeError("replicated() works on device graphs")
        if single.rowptr.numel() != n + 1:
            raise ValueError("a graph with a spare row (the device SAGE rewrite) cannot be replicated")
        g = cls.__new__(cls)
        g.num_nodes, g.num_edges, g.device = n * B, e * B, single.device
        i32 = dict(dtype=torch.int32, device=single.device)
        g.rowptr, g.rowptr_t = torch.empty(n * B + 1, **i32), torch.empty(n * B + 1, **i32)
        g.col, g.eid = torch.empty(e * B, **i32), torch.empty(e * B, **i32)
        g.col_t, g.pos_t, g.eid_t = torch.empty(e * B, **i32), torch.empty(e * B, **i32), torch.empty(e * B, **i32)
        _lib.call("mlgnn_csr_replicate", single.rowptr, single.col, single.eid, single.rowptr_t, single.col_t,
                  single.pos_t, single.eid_t, g.rowptr, g.col, g.eid, g.rowptr_t, g.col_t, g.pos_t, g.eid_t, n, e, B,
                  _lib.stream())
        g._deg, g._scalar_cache, g._table_cache, g._hub = None, None, None, {}
        ev = torch.cuda.Event()
        ev.record()
        g._built = (ev, torch.cuda.current_stream(single.device))
        return g

    def _ordered_after_build(self):
        """A cached graph handed to a stream other than the one its build was enqueued on: that stream waits for the
        build (an event recorded behind it) before any kernel of the caller can read the arrays."""
        ev = getattr(self, "_built", None)
        if ev is not None and torch.cuda.current_stream(self.device) != ev[1]:
            torch.cuda.current_stream(self.device).wait_event(ev[0])
        return self

    def hub_tables(self, direction):
        """Chunk tables of the long rows of one direction (``"dst"``: by-destination CSR, forward; ``"src"``:
        transposed CSR, backward), built on the device on first use: ``(vrows, hubs, counts, capacity)`` or ``None``
        (``HUB_CAP = 0``, a host graph, or no edge)."""
        cap = getattr(self, "hub_cap", HUB_CAP)
        if cap <= 0 or not self.rowptr.is_cuda or self.num_edges == 0:
            return None
        hit = self._hub.get(direction)
        if hit is None and not self._hub:
            # first use: both directions at once -- the backward's tables are then known hub-free (on the host, through
            # the asynchronous count copy) by the time the backward asks, and it skips the empty long-row launches
            # from its first call on
            self._hub[direction] = None
            self.hub_tables("src" if direction == "dst" else "dst")
            del self._hub[direction]
        if hit is None:
            cap_rows = _lib.size("mlgnn_hub_capacity", self.num_edges, cap)
            i32 = dict(dtype=torch.int32, device=self.device)
            vrows, hubs, counts = torch.empty((cap_rows, 3), **i32), torch.empty((cap_rows, 3), **i32), torch.empty(2, **i32)
            rowptr = self.rowptr if direction == "dst" else self.rowptr_t
            _lib.call("mlgnn_hub_rows", rowptr, self.num_nodes, cap, cap_rows, vrows, hubs, counts, _lib.stream())
            # the counts also travel to pinned host memory, asynchronously: once that copy is known to have finished
            # (event.query(), never a wait) a graph without long rows skips the two empty launches per aggregation
            host = torch.empty(2, dtype=torch.int32, pin_memory=True)
            host.copy_(counts, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            hit = self._hub[direction] = [vrows, hubs, counts, cap_rows, host, done, None]
        return hit

    def known_short_rows(self):
        """True once BOTH directions are known on the host -- without ever having waited for it -- to hold no row longer
        than the cap (at most 256 edges): what the compact max backward (csrc/max_sparse.hip) requires."""
        cap = getattr(self, "hub_cap", HUB_CAP)
        if cap <= 0 or cap > 256:
            return False
        for direction in ("dst", "src"):
            tabs = self.hub_tables(direction)
            if tabs is None:
                return False
            if tabs[6] is None and tabs[5].query():
                tabs[6] = int(tabs[4][0]) > 0
            if tabs[6] is not False:
                return False
        return True

    def hub_arg(self, direction, d):
        """``(pointer to a mlgnn_hub_t or None, objects to keep alive until the launch is enqueued)`` for one kernel
        call on ``[N, d]`` features: the tables above plus fresh scratch for the chunks' partial results."""
        tabs = self.hub_tables(direction)
        if tabs is None:
            return None, ()
        if tabs[6] is None and tabs[5].query():
            tabs[6] = int(tabs[4][0]) > 0               # known on the host now, without ever having waited for it
        if tabs[6] is False:
            return None, ()                               # no row longer than HUB_CAP in this direction
        vrows, hubs, counts, cap_rows = tabs[:4]
        tmp, nbytes = _lib.workspace("mlgnn_hub_scratch_bytes", cap_rows, d, device=self.device)
        st = _lib.HubStruct(getattr(self, "hub_cap", HUB_CAP), cap_rows, vrows.data_ptr(), hubs.data_ptr(), counts.data_ptr(), tmp.data_ptr(), nbytes)
        return ctypes.byref(st), (st, tmp)

    def _build_device(self, edge_index):
        """Two stable radix sorts on the GPU (``mlgnn_coo_to_csr``), enqueued on the current stream."""
        N, E, dev = self.num_nodes, self.num_edges, self.device
        ei = edge_index.to(torch.int64).contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        self.rowptr, self.rowptr_t = torch.empty(N + 1, **i32), torch.empty(N + 1, **i32)
        self.col, self.eid = torch.empty(E, **i32), torch.empty(E, **i32)
        self.col_t, self.pos_t, self.eid_t = torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
        ws, nbytes = _lib.workspace("mlgnn_coo_to_csr_workspace_bytes", N, E, device=dev)
        self._bad_ids = torch.empty(1, **i32)               # cleared by the build itself
        _lib.call("mlgnn_coo_to_csr", ei, E, N, self.rowptr, self.col, self.eid, self.rowptr_t, self.col_t, self.pos_t,
                  self.eid_t, self._bad_ids, ws, nbytes, _lib.stream())

    def validate(self):
        """Raise if the edge list named a node outside ``[0, num_nodes)`` (the device build clamps such
        ids and counts them; reading the counter synchronises, so this is opt-in)."""
        bad = getattr(self, "_bad_ids", None)
        if bad is not None and int(bad.item()) != 0:
            raise ValueError("%d edge endpoints outside [0, %d)" % (int(bad.item()), self.num_nodes))
        return self

    def _build_host(self, edge_index):
        """Same layout from torch ops on the CPU: for data-loader workers that pre-sort a batch
        (``batch.csr``) and for the host-side layout tests.  Never used for device tensors."""
        N = self.num_nodes
        src, dst = edge_index[0].long(), edge_index[1].long()
        if edge_index.numel() and (int(edge_index.min()) < 0 or int(edge_index.max()) >= N):
            raise ValueError("edge endpoints outside [0, %d)" % N)
        order = torch.sort(dst, stable=True).indices
        col = src[order]
        order_t = torch.sort(col, stable=True).indices
        self.rowptr = self._ptr(dst, N)
        self.col = col.to(torch.int32)
        self.eid = order.to(torch.int32)
        self.rowptr_t = self._ptr(src, N)
        self.col_t = dst[order][order_t].to(torch.int32)
        self.pos_t = order_t.to(torch.int32)
        self.eid_t = order[order_t].to(torch.int32)

    def to(self, device):
        """Move a host-built graph to the GPU (index arrays only)."""
        for name in ("rowptr", "col", "eid", "rowptr_t", "col_t", "pos_t", "eid_t"):
            setattr(self, name, getattr(self, name).to(device))
        self.device = torch.device(device)
        self._deg, self._scalar_cache, self._table_cache, self._hub = None, None, None, {}
        return self

    @staticmethod
    def _ptr(index, N):
        counts = torch.bincount(index, minlength=N)
        ptr = torch.zeros(N + 1, dtype=torch.int64, device=index.device)
        torch.cumsum(counts, 0, out=ptr[1:])
        return ptr.to(torch.int32)

    @property
    def in_degree(self):
        """float [N]: number of incoming edges (PyG ``degree(index, N)``)."""
        if self._deg is None:
            n = self.num_nodes               # (a SAGE graph carries one spare row behind it)
            self._deg = (self.rowptr[1:n + 1] - self.rowptr[:n]).to(torch.float32)
        return self._deg

    def edge_scalar(self, a):
        """Per-edge scalar [E] (COO order) -> (by-destination order, by-source order).  The last result is kept:
        the entry holds the source tensor itself, so its storage cannot be freed and handed to a different tensor
        with the same address under the cache; a lookup matches any view of the same elements (see :func:`_same_view`)."""
        ent = self._scalar_cache
        if ent is not None and _same_view(ent[0], a) and ent[1] == a._version:
            return ent[2]
        flat = a.reshape(-1).to(torch.float32)
        by_dst = flat[self.eid.long()].contiguous()
        hit = (by_dst, by_dst[self.pos_t.long()].contiguous())
        self._scalar_cache = (a, a._version, hit)
        return hit

    def mean_edge_scalar(self, a=None):
        """Per-edge weights of a MEAN aggregation folded with the 1 / in-degree of the edge's destination:
        ``(w_e / deg(dst_e)`` in by-destination order, the same in by-source order``)`` -- a weighted SUM with these is the
        weighted mean, and its backward is a plain weighted sum without the two row-pointer loads per edge the mean form
        needs for ``deg(dst)`` (a dependent-load chain in a latency-bound kernel).  ``a``: ``[E]`` weights in COO order or
        None (all ones).  Computed once per (graph, weights) and kept: worth it for a graph that outlives the step (the
        fold-constant topology, :func:`shared_sage_graph`)."""
        ent = getattr(self, "_mean_cache", None)
        if ent is not None and ((a is None and ent[0] is None) or (a is not None and ent[0] is not None
                                                                   and _same_view(ent[0], a) and ent[1] == a._version)):
            return ent[2]
        n = self.num_nodes
        deg = (self.rowptr[1:n + 1] - self.rowptr[:n]).to(torch.float32).clamp(min=1.0)
        inv_dst = torch.repeat_interleave(1.0 / deg, (self.rowptr[1:n + 1] - self.rowptr[:n]).long())      # by-destination order
        inv_src = (1.0 / deg)[self.col_t[:inv_dst.numel()].long()]                                          # by-source order
        if a is not None:
            by_dst, by_src = self.edge_table(a, 1)
            hit = ((by_dst.reshape(-1)[:inv_dst.numel()] * inv_dst).contiguous(),
                   (by_src.reshape(-1)[:inv_src.numel()] * inv_src).contiguous())
        else:
            hit = (inv_dst.contiguous(), inv_src.contiguous())
        self._mean_cache = (a, a._version if a is not None else -1, hit)
        return hit

    def edge_table(self, a, width):
        """Per-edge attribute rows [E, r] (COO order) zero padded to ``width`` columns ->
        (by-destination order, by-source order), both [E, width] fp32; cached per tensor."""
        src = a
        if a.dim() == 1:
            a = a[:, None]
        if a.shape[0] != self.num_edges or a.shape[1] > width:
            raise ValueError("edge attributes must be [E=%d, <=%d], got %s" % (self.num_edges, width, tuple(a.shape)))
        ent = self._table_cache
        hit = ent[3] if (ent is not None and _same_view(ent[0], src) and ent[1] == src._version and ent[2] == width) else None
        if hit is None:
            if a.is_cuda and self.eid.is_cuda:
                rows = a if a.dtype == torch.float32 else a.to(torch.float32)
                if rows.stride(1) != 1 and rows.shape[1] > 1:
                    rows = rows.contiguous()
                by_dst = torch.empty((self.num_edges, width), dtype=torch.float32, device=a.device)
                by_src = torch.empty_like(by_dst)
                _lib.call("mlgnn_edge_table_to_csr", rows, rows.stride(0), rows.shape[1], width, self.eid, self.eid_t,
                          by_dst, by_src, self.num_edges, _lib.stream())
                hit = (by_dst, by_src)
            else:
                rows = a.to(torch.float32)
                if rows.shape[1] != width:
                    rows = torch.nn.functional.pad(rows, (0, width - rows.shape[1]))
                by_dst = rows[self.eid.long()].contiguous()
                hit = (by_dst, by_dst[self.pos_t.long()].contiguous())
            self._table_cache = (src, src._version, width, hit)      # holds `src`: see edge_scalar
        return hit


def _content_key(edge_index):
    """(sum of the entries, position-weighted sum) in wrapping int64 arithmetic + the shape: equal index lists give equal
    keys, and two different lists of one shape collide with probability ~2^-64 per word."""
    flat = edge_index.reshape(-1).to(torch.int64)
    w = torch.arange(1, flat.numel() + 1, dtype=torch.int64, device=flat.device) * 0x9E3779B97F4A7C15 % (1 << 62) | 1
    pair = torch.stack([flat.sum(), (flat * w).sum()])
    return tuple(int(v) for v in pair.tolist()) + tuple(edge_index.shape)


def _same_view(held, t):
    """``t`` names exactly the elements of the tensor a cache entry holds: the same object, or another view of the
    same storage with the same offset / shape / strides / dtype (``a[:, 0]`` taken twice gives two objects).  The
    entry keeps ``held`` alive, so an equal address cannot be a recycled allocation; versions are compared by the
    caller (views of one storage share the counter)."""
    if held is t:
        return True
    return (held.dtype == t.dtype and held.device == t.device and held.shape == t.shape
            and held.stride() == t.stride() and held.storage_offset() == t.storage_offset()
            and held.untyped_storage().data_ptr() == t.untyped_storage().data_ptr())


def as_graph(edge_index, num_nodes):
    """Accept a prebuilt :class:`CSRGraph` (e.g. attached by the collate step) or a COO tensor."""
    if isinstance(edge_index, CSRGraph):
        if edge_index.num_nodes != num_nodes:
            raise ValueError("graph has %d nodes, features have %d" % (edge_index.num_nodes, num_nodes))
        return edge_index
    return CSRGraph(edge_index, num_nodes)


_SAGE_CACHE = []          # [(edge_index, edge_attr, N, ei_version, ea_version, graph, weight)]


def _sage_graph_device(edge_index, edge_attr, num_nodes):
    """One kernel writes the rewritten edge list (``mlgnn_sage_rewrite``: self loops parked on a spare node ``N``, the
    ``N`` unit-weight loops appended) instead of the mask / nonzero / two index / two cat launches of the torch form;
    the CSR is built over ``N + 1`` nodes and presented as an ``N``-node graph."""
    E, N = int(edge_index.shape[1]), int(num_nodes)
    ei = edge_index.to(torch.int64).contiguous()
    attr, stride = None, 1
    if edge_attr is not None:
        ea = edge_attr.reshape(edge_attr.shape[0], -1)
        if ea.shape[1] != 1:
            raise ValueError("SAGE edge weights must be scalar per edge")
        attr = ea if ea.dtype == torch.float32 else ea.to(torch.float32)
        stride = attr.stride(0) if E > 0 else 1
    out = torch.empty((2, E + N), dtype=torch.int64, device=ei.device)
    weight = torch.empty(E + N, dtype=torch.float32, device=ei.device) if attr is not None else None
    _lib.call("mlgnn_sage_rewrite", ei, attr, stride, E, N, out, weight, _lib.stream())
    graph = CSRGraph(out, N + 1)
    graph.hub_cap = SAGE_HUB_CAP
    graph.num_nodes = N                      # rowptr / rowptr_t carry one more (unused) row: the parked self loops
    return graph, weight


class SharedTopology:
    """ONE topology carried by every sample of a batch (the reference's loader gives all patients of a fold the same gene
    network, dataloader/multiloader.py:687-691; ``mlgnn.data.Batch.from_data_list`` notices and attaches this object as
    ``batch.shared_topology``): ``edge_index [2, e]`` / ``edge_attr`` of ONE sample (not offset), ``nodes`` per sample,
    ``copies`` samples.  ``key``: the loader-side tensors the device copies were made from -- the identity the per-fold
    caches go by, since the device copies are new tensors in every batch."""

    def __init__(self, edge_index, edge_attr, nodes, copies, key=None):
        self.edge_index, self.edge_attr, self.nodes, self.copies = edge_index, edge_attr, int(nodes), int(copies)
        self.key = key if key is not None else (edge_index, edge_attr)

    def to(self, device, non_blocking=False):
        ea = self.edge_attr.to(device, non_blocking=non_blocking) if self.edge_attr is not None else None
        return SharedTopology(self.edge_index.to(device, non_blocking=non_blocking), ea, self.nodes, self.copies, self.key)


_SHARED_SAGE_CACHE = []      # [(key tensors, versions, nodes, copies, device, with_attr, graph, weight)], most recent first


def shared_sage_graph(shared, device, use_attr=True):
    """SAGEConv's (self-loop rewritten) topology + weights for a batch of ``shared.copies`` samples of ONE graph: the
    single graph is rewritten and sorted once per fold (exact compaction, host-style: one synchronisation, once), the batch
    CSR is its replication (one kernel) -- and both are kept, so a training loop pays NO topology work per step
    (the 10 launches / 0.5 ms of sorting the 64-fold edge list at config/kirc.yaml shape)."""
    k_ei, k_ea = shared.key
    if not use_attr:
        k_ea = None
    vers = (k_ei._version, k_ea._version if k_ea is not None else -1)
    dev = torch.device(device)
    for i, ent in enumerate(_SHARED_SAGE_CACHE):
        if ent[0][0] is k_ei and ent[0][1] is k_ea and ent[1] == vers and ent[2:6] == (shared.nodes, shared.copies, dev,
                                                                                        bool(use_attr)):
            _SHARED_SAGE_CACHE.insert(0, _SHARED_SAGE_CACHE.pop(i))
            return ent[6]._ordered_after_build(), ent[7]
    n, B = shared.nodes, shared.copies
    ei = shared.edge_index.to(dev)
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype, device=dev)
    ei1 = torch.cat([ei[:, keep], loops.unsqueeze(0).expand(2, -1)], dim=1)
    single = CSRGraph(ei1, n)
    graph = CSRGraph.replicated(single, B)
    weight = None
    if use_attr and shared.edge_attr is not None:
        ea = shared.edge_attr.to(dev).reshape(shared.edge_attr.shape[0], -1)
        if ea.shape[1] != 1:
            raise ValueError("SAGE edge weights must be scalar per edge")
        w1 = torch.cat([ea[keep, 0].to(torch.float32), torch.ones(n, device=dev)])
        weight = w1.repeat(B)
    graph.hub_cap = SAGE_HUB_CAP
    graph.persistent = True                   # outlives the step: per-graph tables (mean weights) are worth keeping on it
    _SHARED_SAGE_CACHE.insert(0, ((k_ei, k_ea), vers, n, B, dev, bool(use_attr), graph, weight))
    del _SHARED_SAGE_CACHE[4:]
    return graph, weight


def sage_graph(edge_index, edge_attr, num_nodes, shared=None):
    """Topology + weights SAGEConv propagates over (torch_vertex.py:272-273): existing self loops
    dropped, one self loop of weight 1.0 appended per node.  The layers of one forward pass hand in
    the very same tensors, so the last result is kept (identity + version checked; the cache holds
    the tensors, so their storage cannot be recycled under it)."""
    if isinstance(edge_index, CSRGraph):
        raise TypeError("SAGEConv rewrites self loops: pass the COO edge_index")
    if (shared is not None and _SHARED_TOPOLOGY and edge_index.is_cuda and shared.nodes * shared.copies == num_nodes
            and shared.edge_index.shape[1] * shared.copies == edge_index.shape[1]):
        return shared_sage_graph(shared, edge_index.device, use_attr=edge_attr is not None)
    ea_v = None if edge_attr is None else edge_attr._version
    for ent in _SAGE_CACHE:
        if ent[0] is edge_index and ent[1] is edge_attr and ent[2] == num_nodes and \
                ent[3] == edge_index._version and ent[4] == ea_v:
            return ent[5], ent[6]
    if edge_index.is_cuda:
        graph, weight = _sage_graph_device(edge_index, edge_attr, num_nodes)
    else:
        keep = edge_index[0] != edge_index[1]
        loops = torch.arange(num_nodes, dtype=edge_index.dtype, device=edge_index.device)
        ei = torch.cat([edge_index[:, keep], loops.unsqueeze(0).expand(2, -1)], dim=1)
        weight = None
        if edge_attr is not None:
            ea = edge_attr.reshape(edge_attr.shape[0], -1)
            if ea.shape[1] != 1:
                raise ValueError("SAGE edge weights must be scalar per edge")
            weight = torch.cat([ea[keep, 0].to(torch.float32), torch.ones(num_nodes, device=ea.device)])
        graph = CSRGraph(ei, num_nodes)
    _SAGE_CACHE[:] = [(edge_index, edge_attr, num_nodes, edge_index._version, ea_v, graph, weight)]
    return graph, weight


def _release_at_exit():
    """Topologies, pinned count buffers and events cached at module level are released while torch and the HIP runtime are
    still whole (atexit runs before module teardown): otherwise they are destroyed in arbitrary order during interpreter
    finalisation, next to the runtime's own teardown (one ``terminate called without an active exception`` was seen after
    the last case of tools/fuzz_aggregate.py in round 4, with two cached graphs alive)."""
    try:
        CSRGraph._CACHE[:] = []
        _SAGE_CACHE[:] = []
        _SHARED_SAGE_CACHE[:] = []
        from . import project
        project._MEMBERSHIP_CACHE[:] = []
        from . import pathway_conv
        pathway_conv.PathwayTopology.clear_cache()
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
    except Exception:                                  # noqa: BLE001 -- never turn a clean exit into an error
        pass


import atexit  # noqa: E402
atexit.register(_release_at_exit)
