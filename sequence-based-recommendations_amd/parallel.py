"""Data-parallel training step: the batch rows (independent user sub-sequences, the cost is their
mean: rnn_one_hot.py:71) are sharded over ranks, one process per GPU; every rank computes its
share of cost and gradients (already scaled by 1/B_global inside the engine), the flat gradient
section is summed with an all-reduce (backend "nccl" = RCCL over xGMI on MI355X, "gloo" in the
CPU tests), and every rank applies the identical optimizer step to its replica.

Overlap: the output-layer gradients (W_out, b_out + the cost scalar that rides at the end of the
section) are final after `loss_backward_output`, so their all-reduce is issued right then and runs
while the BPTT chain of `backward_recurrent` executes; the recurrent part follows.  With the HIP
engine every collective is a sync op issued under the engine's SIDE stream (where those gradients are
produced): torch enqueues a sync collective on the current stream, so the main stream goes straight on
to the BPTT chain instead of waiting (`sbr_set_deferred_join`, include/sbr_rnn.h), and no stream of
the process group's own is involved -- a round trip through one cost the step 0.45 ms (train_step).  The sampled heads need the targets of ALL rows on every rank (Blackout's softmax
spans every target column, rnn_sampling.py:68-72,137): `gather_targets` all-gathers B int32.

Row-sparse blocks with the lazy-exact updaters (rmsprop / adadelta / nesterov / adam): a row's missed zero-gradient steps are
replayed when the row is next read, and WHERE that happens splits the replay (a short loop below 32 steps, closed forms above):
calls that bring rows up to date on one rank only -- get_params / save, predict / top-k, flush_lazy -- would let the replicas
drift apart by float32 roundings.  So with more than one rank the engine is GUARDED (`engine.dp_guard`): those calls raise when
made on the engine directly and are offered here as collectives -- `flush_lazy`, `test_function`, `predict_function`,
`get_all_param_values` -- which every rank must enter at the same step (a barrier in front: a rank that enters alone waits for the
others instead of silently forking the replicas; tests/test_dp_gloo.py, tests/test_gpu_dp_two_ranks.py::*_midrun_*).

Where the output layer's all-reduce is issued: small buckets (C2: 1.9 MB) right behind its gradient kernels, on the side stream,
beside the BPTT chain; buckets above `OUT_EARLY_BYTES` (a 26 744 x 256 W_out is 27 MB: ~0.2 ms on a ring over xGMI) would sit in
that stream's queue IN FRONT of the weight-gradient kernels `backward_recurrent` enqueues there and hold them back for as long, so
they are issued behind that work instead, back to back with the recurrent bucket.  The placement relies on a SYNC collective being
ordered on the stream it is issued under (this torch, 2.10, enqueues it there): `_side_collectives_are_ordered` verifies that with
data when a DataParallel with more than one rank is built and otherwise falls back to the fully joined path (`stream_check`); no
>1-GPU box was available to the builder to measure either placement.

The training driver (`python -m sbr_amd.train` under a launcher: `init_from_env`, models.py) adds three things on top of the step:
`train_step_lagged` / `flush_lagged` (the global cost one call late, through sbr_cost_lagged: no wait for the stream per iteration),
`evaluate` (the validation users shared among the ranks behind ONE full flush, the records all-gathered: every rank returns the same
dictionary) and the small broadcasts by which rank 0 decides what all ranks must agree on (initial parameters, seeds, the order of a
pass, the clock where an option consults it).

`engine` is anything with the RNNEngine phase methods -- the CPU tests pass an oracle-backed
stand-in, production passes engine.RNNEngine.
"""


BACKENDS = ("nccl", "gloo")


def env_world(environ=None):
    """WORLD_SIZE of a launcher's job (torch.distributed.run sets it); 1 without one"""
    import os
    return int((os.environ if environ is None else environ).get("WORLD_SIZE", "") or 1)


def device_for_rank(local_rank, n_devices, backend):
    """The device of a rank, as bench.py --dp-backend chooses it: LOCAL_RANK when that device exists; otherwise gloo lets several
    ranks share a device (LOCAL_RANK % device_count) and nccl refuses (RCCL needs one GPU per rank)."""
    if backend not in BACKENDS:
        raise ValueError("SBR_DP_BACKEND=%r: must be one of %s" % (backend, "|".join(BACKENDS)))
    if n_devices < 1:
        raise RuntimeError("data-parallel training runs on the HIP engine: no GPU visible")
    if local_rank < n_devices:
        return local_rank
    if backend == "nccl":
        raise RuntimeError("LOCAL_RANK=%d but %d visible device(s): RCCL needs one GPU per rank (SBR_DP_BACKEND=gloo shares devices)"
                           % (local_rank, n_devices))
    return local_rank % n_devices


def init_from_env(environ=None):
    """The process group of a launcher's job, from RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT; the backend from
    SBR_DP_BACKEND (nccl = RCCL, the default; gloo lets several ranks share one device).  Selects the rank's device and returns
    torch.distributed; None when WORLD_SIZE is unset or 1 (nothing is initialised).  The caller destroys the group."""
    import os
    environ = os.environ if environ is None else environ
    world = env_world(environ)
    if world <= 1:
        return None
    import torch
    import torch.distributed as dist
    rank = int(environ["RANK"])
    backend = environ.get("SBR_DP_BACKEND", "nccl")
    index = device_for_rank(int(environ.get("LOCAL_RANK", rank)), torch.cuda.device_count(), backend)
    torch.cuda.set_device(index)
    init = "tcp://%s:%s" % (environ["MASTER_ADDR"], environ["MASTER_PORT"])
    if backend == "nccl":
        dist.init_process_group("nccl", init_method=init, rank=rank, world_size=world, device_id=torch.device("cuda", index))
    else:
        dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    return dist


class DataParallel(object):
    def __init__(self, engine, dist=None, group=None):
        if dist is None:
            import torch.distributed as dist
        self.engine, self.dist, self.group = engine, dist, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.grads, self.split = engine.section("grads")
        # stream-level overlap needs the engine's side stream and device tensors (RCCL); the gloo CPU tests use a
        # stand-in engine without either
        if self.world > 1 and hasattr(engine, "dp_guard"):
            engine.dp_guard = True                       # rank-local flushes of lazily stepped rows now raise (module docstring)
        self.side = self.side2 = None
        self.tail = None
        self.stream_check = None      # "ordered" / "fallback" / "skipped: ..." once the side-stream placement has been verified
        if hasattr(engine, "side_stream") and getattr(self.grads, "is_cuda", False):
            self.side = engine.side_stream()
            if self.world > 1 and not self._side_collectives_are_ordered():
                # this torch / backend does not order a sync collective behind the stream it is issued under: every collective
                # then runs on the engine's main stream behind a full join (the stand-in path below; correct, nothing overlapped)
                self.side = None
                if not str(self.stream_check or "").startswith("fallback"):
                    self.stream_check = "fallback"
                return
            engine.set_deferred_join(True)
            # overlapped step tail (engine.query("tail_chunks") >= 2): dW_in is finished by the engine's second side stream,
            # dW_hid by the first, everything else of the recurrent part by the main stream -- one collective behind each
            # (query "tail_streams": with SBR_TAIL_OVERLAP=2 the same kernels run on the MAIN stream -- nothing to order behind)
            if hasattr(engine, "side_stream2") and engine.query("tail_streams") == 1:
                self.side2 = engine.side_stream2()
                self.tail = engine.tail_ranges()

    OUT_EARLY_BYTES = 8 << 20      # output-layer buckets up to this size are reduced beside the BPTT chain (module docstring)

    def _side_collectives_are_ordered(self):
        """The step's placement of its collectives rests on ONE property of torch.distributed: a sync collective issued under
        `torch.cuda.stream(side)` consumes what `side` has produced so far and is complete for whatever `side` runs next (torch
        2.10 enqueues it on the current stream; an implementation with a stream of its own must order it by events to the same
        effect).  Checked once per DataParallel, on the real streams, with data: the side stream is held back by a ~1 ms spin,
        then fills a buffer, all-reduces it and copies it -- every call returns to the host long before the spin ends, so a
        collective that did not wait for the side stream would reduce the zeros the buffer still holds.  False -> the caller
        falls back to the fully joined path."""
        try:
            import torch
            t = torch.zeros(8192, device=self.grads.device)
            torch.cuda.synchronize()
            with torch.cuda.stream(self.side):
                torch.cuda._sleep(2000000)
                t.fill_(1.0)
                self.dist.all_reduce(t, group=self.group)
                probe = t.clone()
            torch.cuda.current_stream().wait_stream(self.side)
            torch.cuda.synchronize()
            ok = bool((probe == float(self.world)).all().item())
            note = None
        except Exception as ex:      # (no such private spin kernel in another torch, a backend error on this rank ...): NOTHING was
            ok = False               # verified, so the unverified placement is not used -- and this rank still enters the agreement
            note = "skipped: %r" % (ex,)      # below, so that no rank waits in it alone
        # every rank must take the same path: one that falls back alone would issue its collectives in another order
        import torch
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.grads.device)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN, group=self.group)
        ok = bool(int(flag.item()))
        self.stream_check = "ordered" if ok else ("fallback" if note is None else "fallback (%s)" % note)
        return ok

    # ---- collectives that bring lazily stepped rows up to date: every rank enters them at the same step
    def _collective(self, name, *a, **kw):
        e = self.engine
        if self.world > 1:
            self.dist.barrier(group=self.group)
        e._dp_collective = True
        try:
            return getattr(e, name)(*a, **kw)
        finally:
            e._dp_collective = False

    def flush_lazy(self):
        return self._collective("flush_lazy")

    def test_function(self, *a, **kw):
        return self._collective("test_function", *a, **kw)

    def predict_function(self, *a, **kw):
        return self._collective("predict_function", *a, **kw)

    def get_all_param_values(self):
        return self._collective("get_all_param_values")

    @staticmethod
    def shard(batch_size, world, rank):
        """rows [lo, hi) of the global batch owned by `rank` (contiguous, sizes differ by <= 1)."""
        base, extra = divmod(batch_size, world)
        lo = rank * base + min(rank, extra)
        return lo, lo + base + (1 if rank < extra else 0)

    def gather_targets(self, local_target):
        """all ranks' targets in global row order (equal shard sizes)."""
        if self.world == 1:
            return local_target
        import torch
        parts = [torch.empty_like(local_target) for _ in range(self.world)]
        self.dist.all_gather(parts, local_target, group=self.group)
        return torch.cat(parts)

    def _ranges(self):
        """(output-layer ranges, recurrent ranges) of the gradient section that take the dense all-reduce."""
        if not hasattr(self, "_rng"):
            e = self.engine
            n = self.grads.numel()
            ranges = e.dense_ranges() if hasattr(e, "dense_ranges") else [(0, self.split), (self.split, n)]
            self._rng = ([r for r in ranges if r[0] >= self.split], [r for r in ranges if r[0] < self.split])
            self._nsparse = len(e.sparse_blocks()) if hasattr(e, "sparse_blocks") else 0
        return self._rng

    # Row-sparse blocks whose fixed-capacity exchange buffers stay below this many bytes per rank travel with their row count
    # IN BAND (no host read, nothing synchronised: engine.sparse_pack_device / sparse_unpack_add_all); larger ones keep the
    # counted form -- one 4-byte read-back per block and step against an all-gather of only the rows the step touched (at a
    # 1 M-item catalogue the capacity is T*B_local rows of 8 KB each: there the bytes are the cost, not the read).
    INBAND_BYTES = 32 << 20

    def _exchange_sparse(self, b):
        """Row-sparse block b: all-gather of (row ids, gradient rows) instead of an all-reduce of the whole block
        (8.2 GB of W_in at 1 M items against <= T*B_local rows of it per rank).  Every rank then adds all ranks'
        rows in rank order, so the replicas stay bit-identical."""
        import torch
        e, dist = self.engine, self.dist
        if not hasattr(self, "_sp_info"):
            self._sp_info, self._sp_all = e.sparse_blocks(), {}
        n_rows, width, cap = self._sp_info[b]
        if not hasattr(self, "_sp_same_cap"):
            # the in-band form all-gathers fixed-capacity buffers and strides every rank's slice by THIS rank's capacity: shards
            # that differ by a row can round to different capacities (Bp = local rows rounded up to 16), so the ranks agree once,
            # here, whether all of them hold the same capacity for every block; if not, the counted form serves the block
            caps = torch.tensor([c for _, _, c in self._sp_info], dtype=torch.int64, device=self.grads.device)
            lo, hi = caps.clone(), caps.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
            self._sp_same_cap = [bool(x) for x in (lo == hi).tolist()]
        if hasattr(e, "sparse_pack_device") and self._sp_same_cap[b] and cap * width * 4 <= self.INBAND_BYTES:
            ids, rows = e.sparse_pack_device(b)          # ids[0] = the count; enqueued, not waited for
            if b not in self._sp_all:                     # persistent gather targets: [world][1 + cap], [world][cap][width]
                self._sp_all[b] = (torch.empty((self.world,) + tuple(ids.shape), dtype=ids.dtype, device=ids.device),
                                   torch.empty((self.world,) + tuple(rows.shape), dtype=rows.dtype, device=rows.device))
            ids_all, rows_all = self._sp_all[b]
            dist.all_gather(list(ids_all.unbind(0)), ids, group=self.group)      # (sync ops: on the current stream, see train_step)
            dist.all_gather(list(rows_all.unbind(0)), rows, group=self.group)
            e.sparse_unpack_add_all(b, ids_all, rows_all, self.world)      # one call: rank order, counts read on the device
            return
        ids, rows, n = e.sparse_pack(b)
        cnt = torch.tensor([n], dtype=torch.int32, device=ids.device)
        cnts = [torch.empty_like(cnt) for _ in range(self.world)]
        dist.all_gather(cnts, cnt, group=self.group)
        counts = [int(c) for c in torch.cat(cnts).tolist()]      # (one read-back for all ranks' counts)
        m = max(counts)
        if m == 0:
            return
        ids_m, rows_m = ids[:m].contiguous(), rows[:m].contiguous()
        gids = [torch.empty_like(ids_m) for _ in range(self.world)]
        grows = [torch.empty_like(rows_m) for _ in range(self.world)]
        dist.all_gather(gids, ids_m, group=self.group)
        dist.all_gather(grows, rows_m, group=self.group)
        for r in range(self.world):
            e.sparse_unpack_add(b, gids[r], grows[r], counts[r])

    def _views(self):
        """the slices of the flat gradient section that travel, made once (a slice per step costs ~2 us of host time each)"""
        if not hasattr(self, "_vw"):
            out_r, rec_r = self._ranges()
            g = self.grads
            self._vw = dict(out=[g[lo:hi] for lo, hi in out_r], rec=[g[lo:hi] for lo, hi in rec_r])
        return self._vw

    def train_step(self, exposed=None):
        """One step on the batch already set on the engine; returns nothing (cost: read_cost()).
        exposed: a dict -- the step then brackets the wait for every collective with events on the engine's stream and adds
        the microseconds the stream really stood still for each bucket ("rec": the join behind the side stream's collectives,
        "sparse": the row-sparse exchange; the output layer's collective runs on the side stream and is never waited for alone); a survey mode
        (events cost the stream a few microseconds each: bench.py uses it outside its timed regions)."""
        e = self.engine
        if self.world == 1 and not self.dist.is_initialized():
            e.zero_grads(); e.forward(); e.loss_backward_output(); e.backward_recurrent(); e.apply_update()   # joins inside
            return
        vw = self._views()
        # Collectives are SYNC ops issued under the stream that has to carry them: this torch enqueues a sync collective on the
        # current stream, with no stream of the process group's own and no events.  The async form (the group's stream, an event
        # each way) cost the step +0.45 ms of DEVICE time on one rank -- a record / wait round trip through a foreign stream that
        # shares a hardware queue with one of the engine's (tools/dp_sync_probe.py, profiles/round3_T_dp_sync_probe.txt: through a
        # normal-priority torch stream 0.79 ms, through the engine's own side stream 0.46, the sync op on the engine's stream 0.45
        # against 0.44 without any collective).  One communicator must not run two collectives at once, so all of a step's
        # collectives go to ONE stream: the side stream where there is one (behind the output layer's gradient kernels first,
        # beside the BPTT chain; then behind everything the recurrent part needs), the current stream otherwise.
        red = lambda t: self.dist.all_reduce(t, group=self.group)
        import contextlib
        torch = None
        if self.side is not None:
            import torch
        on_side = (lambda: torch.cuda.stream(self.side)) if self.side is not None else contextlib.nullcontext

        def wait(name, fn):                              # the engine's stream waits: bracketed in survey mode
            if exposed is None or torch is None:
                fn()
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                exposed.setdefault("_ev", []).append((name, e0, e1))
        out_early = sum(t.numel() for t in vw["out"]) * 4 <= self.OUT_EARLY_BYTES
        e.zero_grads()
        e.forward()
        e.loss_backward_output()
        if out_early:
            with on_side():                              # output layer: final now; runs beside the BPTT chain on the side stream
                for t in vw["out"]:
                    red(t)
        e.backward_recurrent()
        if self.side is not None:
            cur = torch.cuda.current_stream()
            if self.tail is None:
                e.join_side()                            # weight-gradient kernels of the recurrent part: the current stream has them
                self.side.wait_stream(cur)
            else:
                # overlapped tail: W_in is finished by the second side stream, W_hid by the first, biases and initial states (the
                # chain's partial sums) by the main stream -- the side stream waits for the other two (sbr_apply_update joins)
                self.side.wait_stream(self.side2)
                self.side.wait_stream(cur)
            with on_side():
                for t in ([] if out_early else vw["out"]) + vw["rec"]:
                    red(t)
            wait("rec", lambda: cur.wait_stream(self.side))
            # row-sparse blocks: packed and unpacked by the engine on ITS stream, so their all-gathers run there too (behind the
            # wait above: one collective of the communicator at a time)
            for b in range(self._nsparse):
                wait("sparse", lambda b=b: self._exchange_sparse(b))
        else:
            for t in ([] if out_early else vw["out"]) + vw["rec"]:
                red(t)
            for b in range(self._nsparse):
                self._exchange_sparse(b)
        e.apply_update()

    # ---- the training loop's form of the step: the cost one call late, without a wait for the stream
    def train_step_lagged(self):
        """train_step() and the cost of the PREVIOUS lagged step (None on the first): after the all-reduce the cost word at the
        end of the gradient section is the global cost, engine.cost_lagged() reports it through pinned memory one call late --
        read_cost() would wait for the stream every iteration.  flush_lagged() returns the last one."""
        self.train_step()
        return self.engine.cost_lagged()

    def flush_lagged(self):
        return self.engine.flush_lagged()

    # ---- what rank 0 decides for all: seeds, the order of a pass, its reading of the clock, the initial parameters
    def _control_device(self):
        """where the small tensors of the broadcasts below live: RCCL moves device memory only, gloo moves host memory"""
        if not hasattr(self, "_ctl"):
            nccl = getattr(self.dist, "get_backend", lambda g=None: "gloo")(self.group) == "nccl"
            self._ctl = self.grads.device if nccl else "cpu"
        return self._ctl

    def broadcast_array(self, array, shape=None, dtype="float64"):
        """rank 0's numpy array on every rank; the others pass None and the shape and dtype they expect"""
        import numpy as np
        if self.world == 1:
            return array
        import torch
        a = np.ascontiguousarray(array) if self.rank == 0 else np.empty(shape, dtype=dtype)
        t = torch.from_numpy(a.reshape(-1)).to(self._control_device())
        self.dist.broadcast(t, src=0, group=self.group)
        return t.cpu().numpy().reshape(a.shape)

    def broadcast_scalar(self, value):
        """rank 0's value (a float64: exact for seeds below 2**53 only -- see broadcast_seed) on every rank"""
        import numpy as np
        return float(self.broadcast_array(np.array([value], dtype=np.float64), (1,), "float64")[0])

    def broadcast_seed(self, seed):
        """rank 0's seed (any int below 2**64) on every rank"""
        import numpy as np
        return int(self.broadcast_array(np.array([int(seed or 0)], dtype=np.uint64).view(np.int64), (1,), "int64").view(np.uint64)[0])

    def broadcast_params(self, values, shapes):
        """rank 0's parameter list (float32 arrays in get_all_param_values order) on every rank: one flat broadcast"""
        import numpy as np
        sizes = [int(np.prod(s)) for s in shapes]
        flat = None if self.rank != 0 else np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in values])
        flat = self.broadcast_array(flat, (sum(sizes),), "float32")
        out, o = [], 0
        for s, n in zip(shapes, sizes):
            out.append(flat[o:o + n].reshape(s)); o += n
        return out

    # ---- validation: every rank evaluates a share of the users, the records are gathered into user order
    def evaluate(self, dataset, users, k, exclude_mode, want_ids=False, want_mask=True):
        """engine.evaluate(dataset, users, ...) as ONE collective: behind a barrier every rank makes a full flush_lazy, evaluates
        users[lo:hi] of its shard and the per-user records are all-gathered into user order (padded to the largest share and
        cut); item_hits is summed.  Every rank returns the same dictionary -- what engine.evaluate returns for the whole list.
        The full flush is what keeps the replicas identical: sbr_evaluate brings current only what it reads (every output row,
        but the W_in rows of its OWN users only), and where a replay of missed steps is split changes float32 roundings (module
        docstring) -- ranks that evaluate different users would leave with different replicas.  After the flush nothing a share
        reads has anything left to replay."""
        import numpy as np
        e = self.engine
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        self._collective("flush_lazy")                   # barrier + the full flush, on every rank
        if self.world == 1:
            e._dp_collective = True
            try:
                return e.evaluate(dataset, users, k, exclude_mode, want_ids=want_ids, want_mask=want_mask)
            finally:
                e._dp_collective = False
        import torch
        n = len(users)
        spans = [self.shard(n, self.world, r) for r in range(self.world)]
        lo, hi = spans[self.rank]
        cap = max(b - a for a, b in spans)
        k = int(k)
        widths = [("n_pred", 1), ("hits", 1), ("first_hit", 1)]
        if want_mask:
            widths.append(("hitmask", (k + 31) // 32))
        if want_ids:
            widths.append(("ids", k))
        n_items = int(e.n_items)
        # one int32 message per rank: `cap` rows of the per-user records side by side, then item_hits
        row = sum(w for _, w in widths)
        msg = np.zeros(cap * row + n_items, dtype=np.int32)
        if hi > lo:                                      # (an empty share makes no engine call: sbr_evaluate rejects n < 1)
            e._dp_collective = True
            try:
                rec = e.evaluate(dataset, users[lo:hi], k, exclude_mode, want_ids=want_ids, want_mask=want_mask)
            finally:
                e._dp_collective = False
            body, o = msg[:cap * row].reshape(cap, row), 0
            for name, w in widths:
                body[:hi - lo, o:o + w] = np.asarray(rec[name]).view(np.int32).reshape(hi - lo, w); o += w
            msg[cap * row:] = rec["item_hits"]
        dev = self._control_device()
        mine = torch.from_numpy(msg).to(dev)
        parts = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(parts, mine, group=self.group)
        parts = [p.cpu().numpy() for p in parts]
        out = {"item_hits": np.zeros(n_items, dtype=np.int32), "hitmask": None, "ids": None}
        cols = {name: [] for name, _ in widths}
        for (a, b), p in zip(spans, parts):
            body, o = p[:cap * row].reshape(cap, row), 0
            for name, w in widths:
                cols[name].append(body[:b - a, o:o + w]); o += w
            out["item_hits"] += p[cap * row:]
        for name, w in widths:
            a = np.ascontiguousarray(np.concatenate(cols[name], axis=0))
            out[name] = a.reshape(n) if name in ("n_pred", "hits", "first_hit") else (a.view(np.uint32) if name == "hitmask" else a)
        return out

    @staticmethod
    def exposed_us(exposed):
        """folds the event pairs train_step(exposed=...) recorded into {bucket: total microseconds}; synchronises"""
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in exposed.pop("_ev", []):
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1) * 1e3
        for k, v in out.items():
            exposed[k] = exposed.get(k, 0.0) + v
        return exposed
