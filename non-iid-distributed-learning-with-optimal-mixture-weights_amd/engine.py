"""Device-resident round engine: HBM layout + the launches of one federated round.

HBM layout (one GPU; see DESIGN.md "Data layout"):
  phi      [rows, ld]   fp32  all local clients' features, CSR by client (row_off), D zero-padded to ld % 64 == 0
  labels   [rows]       int32  (loss='mse': y [rows] fp32 targets instead, the [n, 1] targets flattened)
  row_off  [N+1]        int64
  perms    [E*rows]     int32 this round's shuffles, client j epoch e at E*row_off[j] + e*n_j
  W_out    [N, C, ld]   fp32  the clients x params buffer (each client's trained weights)
  W_g      [C, ld]      fp32  global model
  Z        [n_val, C*ldN] fp32 FedAMW validation logits per client (row v, column c*ldN+n,
                             ldN = N rounded up to 4, padding columns 0)
Everything stays resident across rounds.  Per round the host draws the shuffle
seeds from torch's global CPU generator (one vectorised call) and uploads them
(pinned, double-buffered, async on the compute stream); the permutations themselves
are replayed on the GPU by fs_randperm_device.
"""
import numpy as np
import torch

from . import _lib


def pad_ld(D):
    return max(64, (int(D) + 63) // 64 * 64)


def _to_device_f32(xs, device):
    if len(xs) == 1:
        return xs[0].to(device=device, dtype=torch.float32, non_blocking=True)
    if all(x.is_cuda for x in xs):
        return torch.cat([x.to(device=device, dtype=torch.float32) for x in xs], 0)
    return torch.cat([x.detach().to('cpu', torch.float32) for x in xs], 0).to(device, non_blocking=True)


class Features:
    """Rows of features packed CSR-style in HBM (``phi[rows, ld]``) plus int32 labels --
    or, with ``float_targets`` (the regression task), a float32 ``y[rows]`` buffer instead
    (``labels`` is then None)."""

    def __init__(self, X_list, y_list, D, device, ld=None, float_targets=False):
        self.device = device
        self.D = int(D)
        self.ld = ld or pad_ld(D)
        self.ns = np.array([int(len(y)) for y in y_list], dtype=np.int64)
        self.row_off = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        rows = int(self.row_off[-1])
        self.rows = rows
        for X in X_list:
            if X.dim() != 2 or X.shape[1] != self.D:
                raise ValueError('feature matrix must be [n, D=%d], got %s' % (self.D, tuple(X.shape)))
        self.phi = torch.zeros(max(rows, 1), self.ld, device=device, dtype=torch.float32)
        tdt = torch.float32 if float_targets else torch.int32
        if rows:
            self.phi[:rows, :self.D].copy_(_to_device_f32([torch.as_tensor(x) for x in X_list], device))
            y = torch.cat([torch.as_tensor(v).reshape(-1).to('cpu', torch.float32 if float_targets else torch.int64)
                           for v in y_list])
            tgt = y.to(tdt).to(device)
        else:
            tgt = torch.zeros(1, dtype=tdt, device=device)
        self.labels = None if float_targets else tgt
        self.y = tgt if float_targets else None
        self.targets = tgt
        self.row_off_dev = torch.from_numpy(self.row_off).to(device)


class Shuffler:
    """Shuffles of a fixed set of passes (sizes ns, output offsets offs), replayed on the
    GPU from host-drawn seeds (fs_randperm_device), on whatever stream is current.

    Two output slots let round t+1's shuffles be generated on a side stream while round t
    trains (``prepare``), ordered by events: a slot is rewritten only after the kernel
    that consumed it has finished (``consumed``), and read only after it is ready."""

    def __init__(self, ns, offs, size, device, max_n=None, max_blocks=0):
        self.P = int(len(ns))
        # internal: > 0 replays through fs::randperm_device in the capped, persistent geometry of at
        # most this many workgroups (what the round plan asks for beside a training launch); 0 is
        # fs_randperm_device, the C ABI's geometry
        self.max_blocks = int(max_blocks)
        # the launch contract (include/fedsim.h): max_n bounds every pass; a caller may pass a
        # smaller value only to exercise the error path (check_errors then raises)
        self.max_n = int(max_n) if max_n is not None else (int(np.max(ns)) if self.P else 0)
        self.err = torch.zeros(_lib.ERR_BLOCK // 4, dtype=torch.int32, device=device)
        self.n_dev = torch.as_tensor(np.asarray(ns, dtype=np.int64)).to(device)
        self.off_dev = torch.as_tensor(np.asarray(offs, dtype=np.int64)).to(device)
        self.bufs = [torch.empty(max(1, int(size)), dtype=torch.int32, device=device) for _ in range(2)]
        self.seed_dev = [torch.empty(max(1, self.P), dtype=torch.int64, device=device) for _ in range(2)]
        self.seed_host = [torch.empty(max(1, self.P), dtype=torch.int64, pin_memory=True) for _ in range(2)]
        self.host_free = [None, None]
        self.ready = [None, None]
        self.consumed = [None, None]

    def prepare(self, seeds, slot, stream=None):
        """Enqueue the shuffles for one round into ``bufs[slot]`` on ``stream`` (default: current)."""
        stream = stream or torch.cuda.current_stream()
        seeds = np.asarray(seeds, dtype=np.int64)
        assert seeds.shape == (self.P,)
        if self.host_free[slot] is not None:
            self.host_free[slot].synchronize()
        self.seed_host[slot].numpy()[:] = seeds
        if self.consumed[slot] is not None:
            stream.wait_event(self.consumed[slot])
        with torch.cuda.stream(stream):
            self.seed_dev[slot].copy_(self.seed_host[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            self.host_free[slot] = ev
            if self.P and self.max_blocks > 0:
                _lib.check(_lib.randperm_device_capped()(_lib.ptr(self.seed_dev[slot]), _lib.ptr(self.n_dev),
                                                         _lib.ptr(self.off_dev), self.P, self.max_n,
                                                         _lib.ptr(self.bufs[slot]), _lib.ptr(self.err),
                                                         self.max_blocks, _lib.stream_ptr(stream)),
                           'fs::randperm_device')
            elif self.P:
                _lib.check(_lib.lib().fs_randperm_device(_lib.ptr(self.seed_dev[slot]), _lib.ptr(self.n_dev),
                                                         _lib.ptr(self.off_dev), self.P, self.max_n,
                                                         _lib.ptr(self.bufs[slot]), _lib.ptr(self.err),
                                                         _lib.stream_ptr(stream)),
                           'fs_randperm_device')
            ready = torch.cuda.Event()
            ready.record(stream)
        self.ready[slot] = ready

    def acquire(self, slot):
        """Make the current stream wait for ``bufs[slot]`` and return it."""
        torch.cuda.current_stream().wait_event(self.ready[slot])
        return self.bufs[slot]

    def release(self, slot):
        """Mark ``bufs[slot]`` consumed by the work enqueued so far on the current stream."""
        ev = torch.cuda.Event()
        ev.record()
        self.consumed[slot] = ev

    def run(self, seeds, slot=0):
        """Synchronous-order convenience: prepare on the current stream and return the buffer."""
        self.prepare(seeds, slot)
        return self.acquire(slot)

    def check_errors(self):
        """Raise if a pass broke the max_n contract (it was written unshuffled; synchronises)."""
        err = int(self.err[0].item())
        if err:
            self.err.zero_()
            raise _lib.FedsimError('fs_randperm_device: a pass is longer than max_n = %d; it was written as the '
                                   'identity permutation (code %d)' % (self.max_n, err))


def _check_ws_error(ws, what):
    """Read (synchronising) and clear the sticky error word at the start of the workspace's
    last 256-byte block (include/fedsim.h); raise if a bounded cross-workgroup wait timed out."""
    if ws is None:
        return
    blk = ws[ws.numel() - _lib.ERR_BLOCK:]
    err = int(blk[:4].view(torch.int32).item())
    if err:
        blk.zero_()
        raise _lib.FedsimError('%s: a cross-workgroup hand-off timed out (code %d); results are invalid' % (what, err))


class LocalTrainer:
    """fs_local_train for a fixed set of clients; owns the clients x params buffer.

    ``split``: workgroups per client.  None asks fs_local_train_plan (a group of G
    workgroups splits each client's feature dimension whenever the shape allows, in parallel
    mode as persistent groups over the clients -- two clients per group in the pair form
    (G | _lib.G_PAIR) where the shape allows it -- in chained mode as one group walking the
    chain); 1 forces one workgroup per client, G a split width, G | _lib.G_PAIR the pair form,
    G | _lib.G_TEAMS the team form, G | _lib.G_PIPE the pipelined split form,
    1 | _lib.G_WIDE the batch-tiled form (one workgroup per client, any batch size: what the
    planner answers for B > 64).

    ``loss='mse'`` (the regression task: C = 1, float targets in ``feats``): fs_local_train_mse,
    one workgroup per client, no planner call and no workspace."""

    def __init__(self, feats, C, B, E, split=None, chained=False, rows=None, prox=False, loss='ce'):
        if loss not in ('ce', 'mse'):
            raise ValueError("loss must be 'ce' or 'mse'")
        self.task = loss                  # ('loss' is the trainer's loss buffer below)
        if loss == 'mse' and (int(C) != 1 or feats.y is None):
            raise ValueError("loss='mse' needs C == 1 and Features(float_targets=True)")
        if loss == 'ce' and feats.labels is None:
            raise ValueError("loss='ce' needs integer labels")
        self.f = feats
        self.C, self.B, self.E = int(C), int(B), int(E)
        dev = feats.device
        N = len(feats.ns)
        self.N = N
        self.chained = bool(chained)
        # rows > N: zero padding clients after the real ones (the sharded FedAMW Z block)
        self.W_out = torch.zeros(max(N, int(rows or 0)), self.C, feats.ld, device=dev, dtype=torch.float32)
        self.loss = torch.zeros(N, device=dev, dtype=torch.float64)
        # pass p = j*E + e  ->  (n_j, offset)
        ns = feats.ns
        self.pass_n = np.repeat(ns, self.E)
        self.pass_off = (np.repeat(self.E * feats.row_off[:-1], self.E)
                         + np.tile(np.arange(self.E), N) * np.repeat(ns, self.E)).astype(np.int64)
        self._shuffler = None
        steps = self.E * ((ns + self.B - 1) // self.B)
        order = np.argsort(-steps, kind='stable').astype(np.int32)     # LPT: longest clients dispatched first
        self.order = torch.from_numpy(order).to(dev)
        if loss == 'mse':
            if split not in (None, 1):
                raise _lib.FedsimError('fs_local_train_mse has no split form (one workgroup per client)')
            self.G, self.pair, self.teams, self.pipe, self.width, self.ws = 1, False, False, False, 1, None
            self.wide = False
            return
        import ctypes
        g, wsb = ctypes.c_int(0 if split is None else int(split)), ctypes.c_int64(0)
        max_en = int(self.E * ns.max()) if N else 0
        _lib.check(_lib.lib().fs_local_train_plan(N, self.C, self.B, self.E, feats.ld, max_en, int(self.chained),
                                                  int(bool(prox)), ctypes.byref(g), ctypes.byref(wsb)),
                   'fs_local_train_plan')
        if split is not None and int(split) != g.value:
            raise _lib.FedsimError('fs_local_train_plan: G=%d is not available for this shape (planner: %d)'
                                   % (int(split), g.value))
        self.G = int(g.value)                       # as the ABI takes it (G | G_PAIR: the pair form)
        self.pair = bool(self.G & _lib.G_PAIR)
        self.teams = bool(self.G & _lib.G_TEAMS)
        self.pipe = bool(self.G & _lib.G_PIPE)
        self.wide = bool(self.G & _lib.G_WIDE)      # one workgroup per client, the batch in 64-row blocks
        self.width = self.G & (_lib.G_PAIR - 1)     # workgroups per client group
        self.ws = (torch.zeros(max(2 * _lib.ERR_BLOCK, int(wsb.value)), dtype=torch.uint8, device=dev)
                   if (self.G > 1 or wsb.value > 0) else None)

    def groups(self, cus):
        """Client groups a launch of this trainer runs on ``cus`` CUs (fs_local_train_plan's rule)."""
        if self.G <= 1:
            return 1 if self.chained else self.N
        if self.wide:                      # a persistent grid of at most 512 workgroups walks the clients
            return 1 if self.chained else min(self.N, 512)
        if self.chained:
            return 1
        per = (self.N + 1) // 2 if (self.pair or self.teams) else self.N
        return max(1, min(per, cus // self.width))

    @property
    def shuffler(self):
        """GPU shuffle replay for direct ``run`` calls (the round plan owns its own slots)."""
        if self._shuffler is None:
            self._shuffler = Shuffler(self.pass_n, self.pass_off, self.E * self.f.rows, self.f.device)
        return self._shuffler

    def check_errors(self):
        """Raise if a split-client launch reported a broken hand-off, or a shuffle of this
        trainer's passes broke its length contract (synchronises)."""
        _check_ws_error(self.ws, 'fs_local_train')
        if self._shuffler is not None:
            self._shuffler.check_errors()

    def upload_perms(self, seeds, slot=0, stream=None):
        """seeds: [N*E] sampler seeds of one round's local training passes (client-major);
        the permutations are replayed on the GPU into shuffle slot ``slot``."""
        self.shuffler.prepare(seeds, slot, stream)

    def sel_order(self, sel):
        """The sampled client ids ``sel`` in dispatch order (longest first, stable: the LPT rule
        of ``order`` restricted to them) as an int32 numpy array; validates the ids."""
        sel = np.asarray(sel)
        if sel.ndim != 1 or sel.size < 1 or sel.size > self.N or sel.dtype.kind not in 'iu':
            raise ValueError('sel must be a 1-D array of 1 to %d client ids' % self.N)
        sel = sel.astype(np.int64)
        if int(sel.min()) < 0 or int(sel.max()) >= self.N or len(np.unique(sel)) != sel.size:
            raise ValueError('sel: client ids must be distinct and lie in [0, %d)' % self.N)
        sel = np.sort(sel)
        steps = self.E * ((self.f.ns[sel] + self.B - 1) // self.B)
        return sel[np.argsort(-steps, kind='stable')].astype(np.int32)

    def run(self, W_start, lr, prox, mu, reg, lam, chained, slot=0, loss_out=None, sel=None):
        """Launch local training of every client; ``loss_out`` (float64 [N], default the
        trainer's own buffer) receives the last-epoch losses.

        ``sel`` (client ids; parallel clients only): a subset launch -- the same form over the
        sampled clients alone, through its ``order`` table.  ``W_out[j]`` and ``loss[j]`` stay
        indexed by client id; rows and entries of clients outside ``sel`` are not written."""
        f = self.f
        L = _lib.lib()
        loss = self.loss if loss_out is None else loss_out
        n_run, order = self.N, self.order
        if sel is not None:
            if chained:
                raise ValueError('a subset launch needs parallel clients (chained=False)')
            order = torch.from_numpy(self.sel_order(sel)).to(f.device)
            n_run = int(order.numel())
        perms = self.shuffler.acquire(slot)
        if self.task == 'mse':
            _lib.check(L.fs_local_train_mse(_lib.ptr(f.phi), f.ld, _lib.ptr(f.row_off_dev), _lib.ptr(f.y),
                                            _lib.ptr(perms), None if chained else _lib.ptr(order),
                                            n_run, self.B, self.E, float(lr), float(mu), int(bool(prox)),
                                            float(lam), int(bool(reg)), int(bool(chained)), _lib.ptr(W_start),
                                            _lib.ptr(self.W_out), _lib.ptr(loss), _lib.stream_ptr()),
                       'fs_local_train_mse')
            self.shuffler.release(slot)
            return self.W_out, loss
        _lib.check(L.fs_local_train(_lib.ptr(f.phi), f.ld, _lib.ptr(f.row_off_dev), _lib.ptr(f.labels),
                                    _lib.ptr(perms), None if chained else _lib.ptr(order),
                                    n_run, self.C, self.B, self.E, float(lr), float(mu), int(bool(prox)),
                                    float(lam), int(bool(reg)), int(bool(chained)), _lib.ptr(W_start),
                                    _lib.ptr(self.W_out), _lib.ptr(loss), self.G, _lib.ptr(self.ws),
                                    0 if self.ws is None else self.ws.numel(), _lib.stream_ptr()),
                   'fs_local_train')
        self.shuffler.release(slot)
        return self.W_out, loss

    def run_scaffold(self, W_start, lr, reg, lam, c, ci, slot=0, loss_out=None, sel=None):
        """fs_local_train_scaffold: SCAFFOLD's local training of every client (``sel``: of the
        sampled clients, as ``run``) from ``W_start`` with the server variate ``c`` [C, ld] and the
        client variates ``ci`` [N, C, ld], float32 device tensors; ``ci`` rows of the trained clients
        are replaced by their new variates (option II), in place.  Parallel clients, cross-entropy,
        one workgroup per client whatever ``split`` the trainer was planned with; no prox term."""
        if self.task != 'ce' or self.chained:
            raise ValueError('run_scaffold needs a cross-entropy trainer with parallel clients')
        f = self.f

        def f32(x, n):
            return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= n
        if not (f32(c, self.C * f.ld) and f32(ci, self.N * self.C * f.ld)):
            raise ValueError('run_scaffold: c [C, ld] and ci [N, C, ld] must be contiguous float32 device tensors')
        loss = self.loss if loss_out is None else loss_out
        n_run, order = self.N, self.order
        if sel is not None:
            order = torch.from_numpy(self.sel_order(sel)).to(f.device)
            n_run = int(order.numel())
        perms = self.shuffler.acquire(slot)
        _lib.check(_lib.lib().fs_local_train_scaffold(_lib.ptr(f.phi), f.ld, _lib.ptr(f.row_off_dev),
                                                      _lib.ptr(f.labels), _lib.ptr(perms), _lib.ptr(order), n_run,
                                                      self.C, self.B, self.E, float(lr), float(lam), int(bool(reg)),
                                                      _lib.ptr(W_start), _lib.ptr(c), _lib.ptr(ci),
                                                      _lib.ptr(self.W_out), _lib.ptr(loss), _lib.stream_ptr()),
                   'fs_local_train_scaffold')
        self.shuffler.release(slot)
        return self.W_out, loss


class RoundPlan:
    """fs_plan: the native round driver (csrc/round.hip).  One ``round`` call enqueues a
    round's local training / aggregation / evaluation; ``shuffle`` replays a round's
    training shuffles into a slot on the plan's side stream (GPU replay by default,
    ``shuffle_device=False``: host thread pool + async upload).
    Borrows every device buffer from the objects passed in (they must outlive it)."""

    def __init__(self, trainer, W_g, loss_hist, p=None, aggregator=None, evaluator=None, eval_hist=None,
                 prox=False, mu=0.0, reg=False, lam=0.0, chained=False, shuffle_device=True, host_threads=0,
                 shuffle_after_train=False):
        import ctypes
        f = trainer.f
        self._keep = [trainer, W_g, loss_hist, p, aggregator, evaluator, eval_hist]
        self._h_n = np.ascontiguousarray(f.ns, dtype=np.int64)
        d = _lib.PlanDesc()
        d.d_phi, d.ld, d.d_row_off = f.phi.data_ptr(), f.ld, f.row_off_dev.data_ptr()
        self.loss = trainer.task
        d.loss = 1 if self.loss == 'mse' else 0
        if self.loss == 'mse':
            d.d_y = f.y.data_ptr()
        else:
            d.d_labels = f.labels.data_ptr()
        d.d_order = None if chained else trainer.order.data_ptr()
        d.h_n = self._h_n.ctypes.data
        d.N, d.C, d.B, d.E, d.G = trainer.N, trainer.C, trainer.B, trainer.E, trainer.G
        d.d_ws = None if trainer.ws is None else trainer.ws.data_ptr()
        d.ws_bytes = 0 if trainer.ws is None else trainer.ws.numel()
        d.chained, d.prox, d.reg = int(bool(chained)), int(bool(prox)), int(bool(reg))
        d.mu, d.lam = float(mu), float(lam)
        d.d_W_g, d.d_W_out, d.d_loss_hist = W_g.data_ptr(), trainer.W_out.data_ptr(), loss_hist.data_ptr()
        d.d_p = None if p is None else p.data_ptr()
        if aggregator is not None:
            d.d_agg_ws, d.agg_ws_floats, d.agg_chunks = aggregator.ws.data_ptr(), aggregator.ws.numel(), \
                int(aggregator.chunks)
        if evaluator is not None:
            if evaluator.loss != self.loss:
                raise ValueError('RoundPlan: the evaluator and the trainer disagree on the loss')
            d.d_phi_t, d.n_t = evaluator.f.phi.data_ptr(), evaluator.n
            if self.loss == 'mse':
                d.d_y_t = evaluator.f.y.data_ptr()
            else:
                d.d_labels_t = evaluator.f.labels.data_ptr()
            d.d_eval_ws, d.d_eval_hist = evaluator.ws.data_ptr(), eval_hist.data_ptr()
        d.shuffle_device = int(bool(shuffle_device))
        d.host_threads = int(host_threads)
        d.shuffle_after_train = int(bool(shuffle_after_train))
        self._desc = d
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().fs_plan_create(ctypes.byref(d), ctypes.byref(self._h)), 'fs_plan_create')
        self.npasses = int(trainer.N * trainer.E)

    def set_chunk(self, rounds):
        """Generate the shuffles of ``rounds`` consecutive rounds per launch (device replay;
        before the first ``shuffle``): no cross-stream wait between the rounds of a chunk."""
        _lib.check(_lib.lib().fs_plan_set_shuffle_chunk(self._h, int(rounds)), 'fs_plan_set_shuffle_chunk')

    def eval_blocks(self):
        """Evaluation workgroups a TRAIN launch carries for a deferred evaluation (0: none)."""
        n = _lib.lib().fs_plan_eval_blocks(self._h)
        if n < 0:
            _lib.check(n, 'fs_plan_eval_blocks')
        return n

    def flush(self):
        """Launch a partly collected chunk of shuffles (after a run's last round was prepared)."""
        _lib.check(_lib.lib().fs_plan_shuffle_flush(self._h), 'fs_plan_shuffle_flush')

    def shuffle(self, seeds, t):
        """seeds: [N*E] sampler seeds of round t's training passes (client-major)."""
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        assert seeds.shape == (self.npasses,)
        _lib.check(_lib.lib().fs_plan_shuffle(self._h, seeds.ctypes.data, int(t)), 'fs_plan_shuffle')

    def shuffle_subset(self, seeds, sel, t):
        """fs_plan_shuffle_subset: replay only the passes of the sampled clients ``sel`` (ascending
        ids) of round t; seeds [len(sel) * E], sel-major / epoch-minor."""
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        assert seeds.shape == (sel.size * self._desc.E,)
        _lib.check(_lib.lib().fs_plan_shuffle_subset(self._h, seeds.ctypes.data, sel.ctypes.data, int(sel.size),
                                                     int(t)), 'fs_plan_shuffle_subset')

    def round_subset(self, t, lr, phases, sel, sel_order, q, M=None):
        """fs_plan_round_subset: round t over the sampled clients.  ``sel`` (ascending ids),
        ``sel_order`` (the same ids in dispatch order) int32 and ``q`` float32 are DEVICE tensors
        the launches read asynchronously: the caller keeps them alive and unchanged."""
        M = int(sel.numel()) if M is None else int(M)
        for x, dt in ((sel, torch.int32), (sel_order, torch.int32), (q, torch.float32)):
            if not (x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= M):
                raise ValueError('round_subset: sel / sel_order (int32) and q (float32) must be contiguous device '
                                 'tensors of at least M entries')
        _lib.check(_lib.lib().fs_plan_round_subset(self._h, int(t), float(lr), int(phases), _lib.ptr(sel),
                                                   _lib.ptr(sel_order), _lib.ptr(q), M, _lib.stream_ptr()),
                   'fs_plan_round_subset')

    def set_nova(self, mode, b=None, te=1.0, s0=1.0):
        """fs_plan_set_nova: the rule of the AGGREGATE phases enqueued from now on -- 0 the plain
        aggregate, 1 (``_lib.NOVA_REFERENCE``) / 2 (``_lib.NOVA_UPDATES``) fs_aggregate_nova with the
        round's weights as ``q`` and ``W_g`` as the base.  ``b`` (mode 1): a float32 device tensor the
        launches read asynchronously; the plan keeps the last one alive."""
        if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()):
            raise ValueError('set_nova: b must be a contiguous float32 device tensor')
        _lib.check(_lib.lib().fs_plan_set_nova(self._h, int(mode), None if b is None else _lib.ptr(b), float(te),
                                               float(s0)), 'fs_plan_set_nova')
        self._nova_b = b

    def set_scaffold(self, on, c=None, ci=None, r=None, cs=0.0):
        """fs_plan_set_scaffold: SCAFFOLD rounds from now on -- TRAIN launches
        fs_local_train_scaffold with the server variate ``c`` [C, ld] and the client variates ``ci``
        [N, C, ld], AGGREGATE fs_aggregate_scaffold with the round's weights as ``q``, ``r`` ([N]; [M]
        of a subset round) and ``cs``, updating ``W_g`` and ``c`` in place.  Float32 device tensors the
        launches read asynchronously (the plan keeps the last ones alive).  ``r`` and ``cs`` change
        with the round's lr and sample: call again before each round.  ``on`` false restores the plan."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_scaffold(self._h, 0, None, None, None, 0.0), 'fs_plan_set_scaffold')
            self._scaffold = None
            return
        for x in (c, ci, r):
            if x is not None and not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
                raise ValueError('set_scaffold: c, ci and r must be contiguous float32 device tensors')
        _lib.check(_lib.lib().fs_plan_set_scaffold(self._h, 1, _lib.ptr(c), _lib.ptr(ci), _lib.ptr(r), float(cs)),
                   'fs_plan_set_scaffold')
        self._scaffold = (c, ci, r)

    def set_server_opt(self, rule, m=None, v=None, eta=1.0, beta1=0.0, omb1=1.0, beta2=0.0, omb2=1.0, tau=1.0):
        """fs_plan_set_server_opt: a FedOpt server optimizer on the AGGREGATE phases enqueued from now
        on -- ``rule`` 0 the plain aggregate, ``_lib.OPT_AVGM`` .. ``_lib.OPT_YOGI`` (or their names,
        ``_lib.OPT_RULES``) fs_aggregate_opt with the round's weights as ``q``, updating ``W_g`` and the
        moments ``m`` / ``v`` [C, ld] in place.  TRAIN is unchanged.  Float32 device tensors the
        launches read and write asynchronously (the plan keeps the last ones alive); the scalars are
        float32 values (``tools.server_opt_scalars``)."""
        rule = _lib.OPT_RULES.get(rule, rule) if isinstance(rule, str) else rule
        if not rule:
            _lib.check(_lib.lib().fs_plan_set_server_opt(self._h, 0, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                       'fs_plan_set_server_opt')
            self._server_opt = None
            return
        n = self._desc.C * self._desc.ld
        for x in (m, v):
            if x is not None and not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= n):
                raise ValueError('set_server_opt: m and v must be contiguous float32 device tensors of C * ld floats')
        _lib.check(_lib.lib().fs_plan_set_server_opt(self._h, int(rule), _lib.ptr(m), _lib.ptr(v), float(eta),
                                                     float(beta1), float(omb1), float(beta2), float(omb2), float(tau)),
                   'fs_plan_set_server_opt')
        self._server_opt = (m, v)

    def set_qffl(self, on, g=None, Lc=1.0, S=None, n=None, hc=None, nws=None):
        """fs_plan_set_qffl: q-FedAvg on the AGGREGATE phases enqueued from now on -- fs_aggregate_qffl
        with the round's weights as ``u`` (``qffl_coef``'s, passed as the round's ``p_override`` or the
        subset round's ``q``), ``g`` ([N]; [M] of a subset round, float32), the Lipschitz estimate
        ``Lc``, ``W_g`` in place and the outputs ``S`` [C, ld] float32, ``n`` [N] and ``hc`` [2] float64;
        ``nws``: float64 workspace of ``fs_aggregate_qffl_ws_doubles(N, C * ld)``.  TRAIN is unchanged.
        Device tensors the launches read and write asynchronously (the plan keeps the last ones
        alive).  ``Lc`` follows the round's lr: call again before each round.  ``on`` false restores the
        plain aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_qffl(self._h, 0, None, 0.0, None, None, None, None, 0), 'fs_plan_set_qffl')
            self._qffl = None
            return
        for x, dt in ((g, torch.float32), (S, torch.float32), (n, torch.float64), (hc, torch.float64),
                      (nws, torch.float64)):
            if x is not None and not (x.is_cuda and x.dtype == dt and x.is_contiguous()):
                raise ValueError('set_qffl: g, S (float32), n, hc and nws (float64) must be contiguous device tensors')
        if (S is not None and S.numel() < self._desc.C * self._desc.ld) or (hc is not None and hc.numel() < 2):
            raise ValueError('set_qffl: S needs C * ld floats, hc 2 doubles')
        _lib.check(_lib.lib().fs_plan_set_qffl(self._h, 1, _lib.ptr(g), float(Lc), _lib.ptr(S), _lib.ptr(n),
                                               _lib.ptr(hc), _lib.ptr(nws), 0 if nws is None else nws.numel()),
                   'fs_plan_set_qffl')
        self._qffl = (g, S, n, hc, nws)

    def set_robust(self, on, mode='trimmed_mean', trim=0.1):
        """fs_plan_set_robust: robust aggregation on the AGGREGATE phases enqueued from now on --
        fs_aggregate_robust over the round's rows of ``W_out`` into ``W_g``.  ``mode='trimmed_mean'``:
        b = floor(trim * M) with M the round's own client count (N, or a subset round's M), clamped
        so that 2b < M; ``mode='median'``: b = (M - 1) // 2.  The rule is unweighted: the round's
        weights are ignored.  TRAIN and EVAL are unchanged.  ``on`` false restores the plain aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_robust(self._h, 0, 0, 0.0), 'fs_plan_set_robust')
            return
        modes = {'trimmed_mean': _lib.ROBUST_TRIMMED_MEAN, 'median': _lib.ROBUST_MEDIAN}
        if mode not in modes:
            raise ValueError("set_robust: mode must be 'trimmed_mean' or 'median'")
        _lib.check(_lib.lib().fs_plan_set_robust(self._h, 1, modes[mode], float(trim)), 'fs_plan_set_robust')

    def set_krum(self, on, f=0.1, m=0, pick=None, score=None, ws=None):
        """fs_plan_set_krum: Krum / Multi-Krum on the AGGREGATE phases enqueued from now on --
        fs_aggregate_krum over the round's rows of ``W_out`` with x = ``W_g`` into ``W_g``.  ``f``: the
        Byzantine fraction in [0, 0.5), f = min(floor(f * M), (M - 3) // 2) with M the round's own
        client count; ``m``: 1 Krum, 0 Multi-Krum (M - f), else a count clamped to M - f.  ``pick``
        int32 [N] and ``score`` float64 [N] take every round's picked ids (the first m entries) and
        scores (by position); ``ws``: ``Aggregator.krum_ws()`` (uint8), the distance matrix at its
        start.  The weights are ignored, TRAIN and EVAL are unchanged.  ``on`` false restores the plain
        aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_krum(self._h, 0, 0.0, 0, None, None, None, 0), 'fs_plan_set_krum')
            self._krum = None
            return
        if not (pick is not None and pick.is_cuda and pick.dtype == torch.int32 and pick.is_contiguous()
                and score is not None and score.is_cuda and score.dtype == torch.float64 and score.is_contiguous()
                and ws is not None and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
            raise ValueError('set_krum: pick (int32), score (float64) and ws (uint8) must be contiguous device tensors')
        _lib.check(_lib.lib().fs_plan_set_krum(self._h, 1, float(f), int(m), _lib.ptr(pick), _lib.ptr(score),
                                               _lib.ptr(ws), ws.numel()), 'fs_plan_set_krum')
        self._krum = (pick, score, ws)

    def set_rfa(self, on, iters=3, nu=1e-6, init='start', uniform=False, dist=None, b=None, obj=None, ws=None):
        """fs_plan_set_rfa: RFA on the AGGREGATE phases enqueued from now on -- fs_aggregate_rfa over the
        round's rows of ``W_out`` with x = ``W_g`` into ``W_g``: ``iters`` smoothed Weiszfeld iterations with
        the smoothing ``nu`` from ``init`` ('start': ``W_g``; 'mean': the finite rows' weighted mean), under
        the round's weights or, with ``uniform``, 1 / M.  ``dist`` float64 [N], ``b`` float32 [N] and ``obj``
        float64 [iters + 2] take every round's distances to the new ``W_g``, last weights (by position) and
        objectives; ``ws``: ``Aggregator.rfa_ws()`` (uint8).  TRAIN and EVAL are unchanged.  ``on`` false
        restores the plain aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_rfa(self._h, 0, 0, 0.0, 0, 0, None, None, None, None, 0),
                       'fs_plan_set_rfa')
            self._rfa = None
            return
        if init not in RFA_INITS:
            raise ValueError("set_rfa: init must be 'start' or 'mean'")
        if not (dist is not None and dist.is_cuda and dist.dtype == torch.float64 and dist.is_contiguous()
                and b is not None and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()
                and obj is not None and obj.is_cuda and obj.dtype == torch.float64 and obj.is_contiguous()
                and obj.numel() >= int(iters) + 2
                and ws is not None and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
            raise ValueError('set_rfa: dist (float64), b (float32), obj (float64 [iters + 2]) and ws (uint8) must be '
                             'contiguous device tensors')
        _lib.check(_lib.lib().fs_plan_set_rfa(self._h, 1, int(iters), float(nu), RFA_INITS[init], int(bool(uniform)),
                                              _lib.ptr(dist), _lib.ptr(b), _lib.ptr(obj), _lib.ptr(ws), ws.numel()),
                   'fs_plan_set_rfa')
        self._rfa = (dist, b, obj, ws)

    def set_topk(self, on, kcount=1, e=None, tau=None, kept=None, ws=None):
        """fs_plan_set_topk: FedTopK on the AGGREGATE phases enqueued from now on -- fs_aggregate_topk over
        the round's rows of ``W_out`` with the round's weights, ``W_g`` in place: every row's corrected
        update thresholded at its ``kcount``-th largest magnitude (ties kept), the kept part folded onto
        ``W_g``, the rest left in the client's row of ``e`` float32 [N, C * ld] (None: no memory, the
        rest is dropped).  ``tau`` float32 [N] and ``kept`` int32 [N] take every round's thresholds (the
        key's bits) and kept counts (by position); ``ws``: ``Aggregator.topk_ws()`` (uint8) or None.
        TRAIN and EVAL are unchanged.  ``on`` false restores the plain aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_topk(self._h, 0, 0, None, None, None, None, 0), 'fs_plan_set_topk')
            self._topk = None
            return
        if not (tau is not None and tau.is_cuda and tau.dtype == torch.float32 and tau.is_contiguous()
                and kept is not None and kept.is_cuda and kept.dtype == torch.int32 and kept.is_contiguous()
                and (e is None or (e.is_cuda and e.dtype == torch.float32 and e.is_contiguous()))
                and (ws is None or (ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()))):
            raise ValueError('set_topk: tau (float32), kept (int32), e (float32 or None) and ws (uint8 or None) must '
                             'be contiguous device tensors')
        _lib.check(_lib.lib().fs_plan_set_topk(self._h, 1, int(kcount), _lib.ptr(e), _lib.ptr(tau), _lib.ptr(kept),
                                               _lib.ptr(ws), 0 if ws is None else ws.numel()), 'fs_plan_set_topk')
        self._topk = (e, tau, kept, ws)

    def set_dp(self, on, clip=1.0, noise_multiplier=0.0, seed=0, uniform=False, adaptive=None, clip_dev=None,
               c=None, r=None, state=None, ws=None, cols=None):
        """fs_plan_set_dp: DP-FedAvg on the AGGREGATE phases enqueued from now on -- fs_aggregate_dp over the
        round's rows of ``W_out`` with the round's weights (``uniform``: 1 / M), ``W_g`` in place: every update
        clipped to the norm ``clip``, the clipped updates folded onto ``W_g`` and Gaussian noise of standard
        deviation ``noise_multiplier * clip * max_k q_k`` added from the Philox field of (``seed``, the round
        call's t).  ``adaptive``: None or dict(quantile, lr, count_noise); the clip then lives in ``clip_dev``
        (float64 [1], set to ``clip`` by the caller before the first round) and is updated on the device.
        ``c`` float32 [N], ``r`` float64 [N] and ``state`` float64 [DP_STATE] take every round's coefficients,
        update norms (by position) and state; ``ws``: ``Aggregator.dp_ws()`` (uint8); ``cols``: D, the model's
        real columns (the padding up to ld takes no noise).  TRAIN and EVAL are unchanged.  ``on`` false restores the plain aggregate."""
        if not on:
            _lib.check(_lib.lib().fs_plan_set_dp(self._h, 0, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, 0.0, None, 0, None, None,
                                                 None, None, 0), 'fs_plan_set_dp')
            self._dp = None
            return

        def ok(x, dt):
            return x is not None and x.is_cuda and x.dtype == dt and x.is_contiguous()
        if not (ok(c, torch.float32) and ok(r, torch.float64) and ok(state, torch.float64)
                and state.numel() >= DP_STATE and ok(ws, torch.uint8)
                and (adaptive is None or (ok(clip_dev, torch.float64) and clip_dev.numel() >= 1))):
            raise ValueError('set_dp: c (float32), r, state (float64), ws (uint8) and, with adaptive, clip_dev '
                             '(float64) must be contiguous device tensors')
        ad = dict(adaptive or {})
        _lib.check(_lib.lib().fs_plan_set_dp(self._h, 1, float(clip), float(noise_multiplier), int(seed),
                                             int(bool(uniform)), int(adaptive is not None),
                                             float(ad.get('quantile', 0.0)), float(ad.get('lr', 0.0)),
                                             float(ad.get('count_noise', 0.0)),
                                             _lib.ptr(clip_dev) if adaptive is not None else None, int(cols),
                                             _lib.ptr(c), _lib.ptr(r), _lib.ptr(state), _lib.ptr(ws), ws.numel()),
                   'fs_plan_set_dp')
        self._dp = (clip_dev, c, r, state, ws)

    def eval_flush(self):
        """fs_plan_eval_flush (ABI 15): complete any evaluation still deferred, so the eval
        history is final on the current stream."""
        _lib.check(_lib.lib().fs_plan_eval_flush(self._h, _lib.stream_ptr()), 'fs_plan_eval_flush')

    def round(self, t, lr, phases, p_override=None):
        _lib.check(_lib.lib().fs_plan_round(self._h, int(t), float(lr), int(phases),
                                            None if p_override is None else _lib.ptr(p_override),
                                            _lib.stream_ptr()), 'fs_plan_round')

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.fs_plan_destroy(h)
            self._h = None


class Aggregator:
    """fs_aggregate over a clients x params buffer."""

    def __init__(self, N, C, ld, device, chunks=0):
        self.N, self.len = int(N), int(C) * int(ld)
        self.chunks = chunks
        maxc = max(1, min(64, self.N))
        self.ws = torch.empty(maxc * self.len, dtype=torch.float32, device=device)

    def run(self, W_all, p, out):
        _lib.check(_lib.lib().fs_aggregate(_lib.ptr(W_all), self.len, _lib.ptr(p), self.N, self.len, _lib.ptr(out),
                                           _lib.ptr(self.ws), self.ws.numel(), int(self.chunks), _lib.stream_ptr()),
                   'fs_aggregate')
        return out

    def run_sel(self, W_all, sel, q, out, check=True):
        """fs_aggregate_sel: ``out = sum_k q[k] * W_all[sel[k]]`` in k order, bitwise ``run`` on the
        compacted copy ``W_all[sel]`` (an Aggregator of len(sel) clients with the same ``chunks``
        and workspace).  ``sel`` int32 and ``q`` float32: device tensors of equal length; rows of
        ``W_all`` outside ``sel`` are never read.  ``check`` reads ``sel`` back to hold it to the rows
        of ``W_all`` (it synchronises; ``check=False`` for a ``sel`` validated before, as in a timed
        loop -- nothing on the device checks the ids)."""
        M = int(sel.numel())
        if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and q.is_cuda
                and q.dtype == torch.float32 and q.is_contiguous() and q.numel() == M and M >= 1):
            raise ValueError('run_sel: sel (int32) and q (float32) must be contiguous device tensors of equal, '
                             'non-zero length')
        if check:
            rows = W_all.numel() // self.len
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_sel: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_sel(_lib.ptr(W_all), self.len, _lib.ptr(sel), _lib.ptr(q), M, self.len,
                                               _lib.ptr(out), _lib.ptr(self.ws), self.ws.numel(), int(self.chunks),
                                               _lib.stream_ptr()), 'fs_aggregate_sel')
        return out


    def run_nova(self, W_all, q, out, mode, b=None, te=1.0, s0=1.0, base=None, sel=None, check=True):
        """fs_aggregate_nova: FedNova's scaled fold over the rows ``sel`` of ``W_all`` (None: rows
        0..len(q)-1) in k order, in the regimes of ``run`` at len(q) clients.  mode 1
        (``_lib.NOVA_REFERENCE``): ``out = W[sel_0]*s0 + sum_{k>=1} ((q_k*W[sel_k])*te)/b_k``, the
        reference's lines; mode 2 (``_lib.NOVA_UPDATES``): ``out = base + sum_k q_k*(W[sel_k] - base)``,
        where ``base`` may be ``out``.  ``check`` as in ``run_sel``."""
        M = int(q.numel())

        def f32(x):
            return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if not (f32(q) and M >= 1 and (b is None or (f32(b) and b.numel() == M))
                and (base is None or (f32(base) and base.numel() >= self.len))):
            raise ValueError('run_nova: q, b (float32, equal non-zero length) and base (float32, len) must be '
                             'contiguous device tensors')
        if sel is not None:
            if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == M):
                raise ValueError('run_nova: sel must be a contiguous int32 device tensor as long as q')
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('run_nova: q is longer than W_all has rows')
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_nova: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_nova(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                                _lib.ptr(q), None if b is None else _lib.ptr(b), float(te), float(s0),
                                                int(mode), None if base is None else _lib.ptr(base), M, self.len,
                                                _lib.ptr(out), _lib.ptr(self.ws), self.ws.numel(), int(self.chunks),
                                                _lib.stream_ptr()), 'fs_aggregate_nova')
        return out

    def run_scaffold(self, W_all, q, r, cs, W_g, c, sel=None, check=True):
        """fs_aggregate_scaffold: SCAFFOLD's server step from one pass over the rows ``sel`` of
        ``W_all`` (None: rows 0..len(q)-1), both in place with x = ``W_g`` on entry:
        ``W_g = x + sum_k q_k*(W_k - x)`` -- bitwise ``run_nova`` mode 2 on a workspace of half the
        size -- and ``c = cs*c + sum_k r_k*(x - W_k)``, in the regimes of ``run`` at len(q) clients.
        ``check`` as in ``run_sel``."""
        M = int(q.numel())

        def f32(x):
            return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if not (f32(q) and f32(r) and M >= 1 and r.numel() == M and f32(W_g) and f32(c)
                and W_g.numel() >= self.len and c.numel() >= self.len):
            raise ValueError('run_scaffold: q, r (float32, equal non-zero length), W_g and c (float32, len) must be '
                             'contiguous device tensors')
        if sel is not None:
            if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == M):
                raise ValueError('run_scaffold: sel must be a contiguous int32 device tensor as long as q')
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('run_scaffold: q is longer than W_all has rows')
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_scaffold: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_scaffold(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                                    _lib.ptr(q), _lib.ptr(r), float(cs), M, self.len, _lib.ptr(W_g),
                                                    _lib.ptr(c), _lib.ptr(self.ws), self.ws.numel(), int(self.chunks),
                                                    _lib.stream_ptr()), 'fs_aggregate_scaffold')
        return W_g, c

    def run_opt(self, W_all, q, rule, W_g, m, v=None, eta=1.0, beta1=0.0, omb1=1.0, beta2=0.0, omb2=1.0, tau=1.0,
                sel=None, check=True):
        """fs_aggregate_opt: the FedOpt server step from one pass over the rows ``sel`` of ``W_all``
        (None: rows 0..len(q)-1), in place with x = ``W_g`` on entry: ``delta = sum_k q_k*(W_k - x)``
        folded as ``run_nova`` mode 2 folds it (the regimes of ``run`` at len(q) clients), then the
        step of ``rule`` (``_lib.OPT_AVGM`` .. ``_lib.OPT_YOGI`` or a name of ``_lib.OPT_RULES``) on ``W_g``
        and the moments ``m``, ``v`` (None for avgm).  The scalars are passed as float32 values
        (``tools.server_opt_scalars``).  ``check`` as in ``run_sel``."""
        M = int(q.numel())
        rule = _lib.OPT_RULES.get(rule, rule) if isinstance(rule, str) else rule

        def f32(x):
            return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if not (f32(q) and M >= 1 and all(x is None or (f32(x) and x.numel() >= self.len) for x in (W_g, m, v))):
            raise ValueError('run_opt: q (float32, non-zero length), W_g, m and v (float32, len) must be contiguous '
                             'device tensors')
        if sel is not None:
            if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == M):
                raise ValueError('run_opt: sel must be a contiguous int32 device tensor as long as q')
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('run_opt: q is longer than W_all has rows')
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_opt: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_opt(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                               _lib.ptr(q), int(rule), float(eta), float(beta1), float(omb1),
                                               float(beta2), float(omb2), float(tau), M, self.len, _lib.ptr(W_g),
                                               _lib.ptr(m), _lib.ptr(v), _lib.ptr(self.ws), self.ws.numel(),
                                               int(self.chunks), _lib.stream_ptr()), 'fs_aggregate_opt')
        return W_g, m, v

    def qffl_ws(self, M=None):
        """A float64 workspace for ``run_qffl`` at ``M`` rows (fs_aggregate_qffl_ws_doubles); None: for
        any M up to N, what ``RoundPlan.set_qffl`` asks for (the table is largest at the last M of a
        regime of the fold, not always at N)."""
        need = _lib.lib().fs_aggregate_qffl_ws_doubles
        Ms = [int(M)] if M is not None else [self.N] + [m for m in (15, 23, 47, 95, 191, 512) if m < self.N]
        return torch.empty(max(1, max(int(need(m, self.len)) for m in Ms)), dtype=torch.float64, device=self.ws.device)

    def run_qffl(self, W_all, u, g, Lc, W_g, S, n, hc, nws, sel=None, check=True):
        """fs_aggregate_qffl: the q-FedAvg server step from one pass over the rows ``sel`` of ``W_all``
        (None: rows 0..len(u)-1), with x = ``W_g`` on entry: ``S = sum_k u_k*(W_k - x)`` folded as
        ``run_opt`` folds its delta, ``n[k] = ||W_k - x||^2`` (float64) from the same loads,
        ``H = Lc*sum(u) + sum(g*n)``, ``coef = f32(Lc / H)`` (0 when H is not finite or <= 0),
        ``W_g += coef * S`` in place, ``hc = (H, coef)``.  ``u``, ``g``, ``W_g``, ``S`` float32; ``n`` [len(u)],
        ``hc`` [2], ``nws`` (``qffl_ws``) float64.  ``check`` as in ``run_sel``."""
        M = int(u.numel())

        def ok(x, dt, cnt):
            return x is not None and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= cnt
        if not (M >= 1 and ok(u, torch.float32, M) and ok(g, torch.float32, M) and ok(W_g, torch.float32, self.len) and
                ok(S, torch.float32, self.len) and ok(n, torch.float64, M) and ok(hc, torch.float64, 2) and
                ok(nws, torch.float64, 1)):
            raise ValueError('run_qffl: u, g (float32, the same non-zero length), W_g, S (float32, len), n, hc and '
                             'nws (float64) must be contiguous device tensors')
        if sel is not None:
            if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == M):
                raise ValueError('run_qffl: sel must be a contiguous int32 device tensor as long as u')
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('run_qffl: u is longer than W_all has rows')
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_qffl: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_qffl(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                                _lib.ptr(u), _lib.ptr(g), float(Lc), M, self.len, _lib.ptr(W_g),
                                                _lib.ptr(S), _lib.ptr(n), _lib.ptr(hc), _lib.ptr(self.ws),
                                                self.ws.numel(), int(self.chunks), _lib.ptr(nws), nws.numel(),
                                                _lib.stream_ptr()), 'fs_aggregate_qffl')
        return W_g, S, n, hc

    def krum_ws(self, M=None):
        """A uint8 workspace for ``run_krum`` / ``krum_distances`` at up to ``M`` rows (None: N):
        fs_aggregate_krum_ws_bytes, what ``RoundPlan.set_krum`` asks for."""
        M = self.N if M is None else int(M)
        return torch.empty(max(16, int(_lib.lib().fs_aggregate_krum_ws_bytes(M, self.len))), dtype=torch.uint8,
                           device=self.ws.device)

    def _krum_rows(self, what, W_all, x, sel, check):
        M = self.N if sel is None else int(sel.numel())
        if not (W_all.is_cuda and W_all.dtype == torch.float32 and W_all.is_contiguous() and x.is_cuda
                and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= self.len):
            raise ValueError('%s: W_all and x must be contiguous float32 device tensors' % what)
        if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and M >= 1):
            raise ValueError('%s: sel must be a contiguous, non-empty int32 device tensor' % what)
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('%s: W_all has fewer than N rows' % what)
        if M > krum_max_m():
            raise ValueError('%s: M = %d is above fs_aggregate_krum_max_m() = %d' % (what, M, krum_max_m()))
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('%s: sel must index rows of W_all, [0, %d)' % (what, rows))
        return M

    def krum_distances(self, W_all, x, D, ws, sel=None, check=True):
        """fs_krum_distances: ``D`` float32 [M, krum_ldd(M)] = the squared distances between the rows
        ``sel`` of ``W_all`` (None: rows 0..N-1), each centred on ``x`` first (include/fedsim.h: the order
        and the bound).  ``ws``: ``krum_ws()``.  Exactly symmetric, a zero diagonal, +Inf where a
        distance is not finite; the padding columns are left as they are."""
        M = self._krum_rows('krum_distances', W_all, x, sel, check)
        if not (D.is_cuda and D.dtype == torch.float32 and D.is_contiguous() and D.numel() >= M * krum_ldd(M)
                and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
            raise ValueError('krum_distances: D (float32 [M, ldD]) and ws (uint8) must be contiguous device tensors')
        _lib.check(_lib.lib().fs_krum_distances(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                                self.len, _lib.ptr(x), _lib.ptr(D), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_ptr()), 'fs_krum_distances')
        return D

    def run_krum(self, W_all, x, f, m, out, pick, score, ws, sel=None, check=True):
        """fs_aggregate_krum: Krum (``m = 1``) / Multi-Krum over the rows ``sel`` of ``W_all`` (None: rows
        0..N-1) about the round-start model ``x`` with the Byzantine bound ``f``: the pairwise squared
        distances of the centred rows, every row's score (the sum of its M - f - 2 smallest distances,
        float64 into ``score`` [M]), the m rows of the smallest (score, position) (their row ids into
        ``pick`` [m], int32) and their uniform mean into ``out`` -- bitwise ``run_sel(W_all, pick, 1/m)``.
        ``out`` may be ``x``.  ``ws``: ``krum_ws()``; the distance matrix stands at its start afterwards
        (float32 [M, krum_ldd(M)]).  ``check`` as in ``run_sel``."""
        M = self._krum_rows('run_krum', W_all, x, sel, check)
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= self.len
                and pick.is_cuda and pick.dtype == torch.int32 and pick.is_contiguous() and pick.numel() >= max(1, int(m))
                and score.is_cuda and score.dtype == torch.float64 and score.is_contiguous() and score.numel() >= M
                and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
            raise ValueError('run_krum: out (float32), pick (int32 [m]), score (float64 [M]) and ws (uint8) must be '
                             'contiguous device tensors')
        _lib.check(_lib.lib().fs_aggregate_krum(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                                self.len, _lib.ptr(x), int(f), int(m), _lib.ptr(out), _lib.ptr(pick),
                                                _lib.ptr(score), _lib.ptr(ws), ws.numel(), _lib.ptr(self.ws),
                                                self.ws.numel(), int(self.chunks), _lib.stream_ptr()),
                   'fs_aggregate_krum')
        return out

    def rfa_ws(self, M=None):
        """A uint8 workspace for ``run_rfa`` at up to ``M`` rows (None: N): fs_aggregate_rfa_ws_bytes, what
        ``RoundPlan.set_rfa`` asks for."""
        return torch.empty(max(16, rfa_ws_bytes(self.N if M is None else int(M), self.len)), dtype=torch.uint8,
                           device=self.ws.device)

    def run_rfa(self, W_all, x, alpha, T, nu, init, out, dist, b, obj, ws, sel=None, check=True):
        """fs_aggregate_rfa: RFA over the rows ``sel`` of ``W_all`` (None: rows 0..N-1) -- ``T`` smoothed
        Weiszfeld iterations (smoothing ``nu``) towards their geometric median under the weights ``alpha``
        (float32 [M]), from ``init`` = 'start' (the round-start model ``x``) or 'mean' (the finite rows'
        weighted mean), into ``out`` (may be ``x``).  ``dist`` float64 [M]: the distances to ``out``; ``b``
        float32 [M]: the last weights used; ``obj`` float64 [T + 2]: the smoothed objective at every iterate
        (NaN in the slots the chain does not reach).  ``ws``: ``rfa_ws()``.  The rule and its orders:
        include/fedsim.h.  ``check`` as in ``run_sel``."""
        M = self._krum_rows('run_rfa', W_all, x, sel, False)
        if M > rfa_max_m():
            raise ValueError('run_rfa: M = %d is above fs_aggregate_rfa_max_m() = %d' % (M, rfa_max_m()))
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= W_all.numel() // self.len:
                raise ValueError('run_rfa: sel must index rows of W_all, [0, %d)' % (W_all.numel() // self.len))
        if init not in RFA_INITS:
            raise ValueError("run_rfa: init must be 'start' or 'mean'")
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= self.len
                and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.is_contiguous() and alpha.numel() >= M
                and dist.is_cuda and dist.dtype == torch.float64 and dist.is_contiguous() and dist.numel() >= M
                and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() >= M
                and obj.is_cuda and obj.dtype == torch.float64 and obj.is_contiguous()
                and obj.numel() >= max(0, int(T)) + 2
                and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
            raise ValueError('run_rfa: out, alpha [M], b [M] (float32), dist [M], obj [T + 2] (float64) and ws (uint8) '
                             'must be contiguous device tensors')
        _lib.check(_lib.lib().fs_aggregate_rfa(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                               self.len, _lib.ptr(x), _lib.ptr(alpha), int(T), float(nu),
                                               RFA_INITS[init], _lib.ptr(out), _lib.ptr(dist), _lib.ptr(b),
                                               _lib.ptr(obj), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   'fs_aggregate_rfa')
        return out

    def topk_ws(self, M=None):
        """A uint8 workspace for ``run_topk`` / ``topk_threshold`` at up to ``M`` rows (None: N):
        fs_aggregate_topk_ws_bytes (the select keeps its counts in LDS: 0 bytes, a 16-byte tensor)."""
        return torch.empty(max(16, topk_ws_bytes(self.N if M is None else int(M), self.len)), dtype=torch.uint8,
                           device=self.ws.device)

    def _topk_args(self, what, W_all, W_g, e, kcount, tau, kept, ws, sel, M, check):
        def ok(x, dt, cnt):
            return x is not None and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= cnt
        rows = W_all.numel() // self.len
        if not (M >= 1 and ok(W_all, torch.float32, self.len) and ok(W_g, torch.float32, self.len)
                and ok(tau, torch.float32, M) and ok(kept, torch.int32, M)
                and (e is None or ok(e, torch.float32, rows * self.len))
                and (ws is None or ok(ws, torch.uint8, topk_ws_bytes(M, self.len)))):
            raise ValueError('%s: W_all, W_g (float32), tau (float32 [M]), kept (int32 [M]), e (float32, as large as '
                             'W_all, or None) and ws (uint8 or None) must be contiguous device tensors' % what)
        if isinstance(kcount, bool) or not isinstance(kcount, (int, np.integer)) or not 1 <= kcount <= self.len:
            raise ValueError('%s: kcount must be an int in [1, %d]' % (what, self.len))
        if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous()
                                    and sel.numel() == M):
            raise ValueError('%s: sel must be a contiguous int32 device tensor of M ids' % what)
        if sel is None and M > rows:
            raise ValueError('%s: W_all has fewer than M rows' % what)
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('%s: sel must index rows of W_all, [0, %d)' % (what, rows))

    def topk_threshold(self, W_all, W_g, e, kcount, tau, kept, sel=None, M=None, ws=None, check=True):
        """fs_topk_threshold: stage A of ``run_topk`` over the rows ``sel`` of ``W_all`` (None: rows
        0..M-1, M = N unless given) -- every row's corrected update a_k = (W_k - W_g) + e_k, its
        ``kcount``-th largest magnitude key into ``tau`` (float32 [M], the key's bits) and the count of
        keys at or above it into ``kept`` (int32 [M]).  With ``e`` (float32, rows as ``W_all``) it leaves
        a_k IN e_k; ``e`` None: no memory, a_k = W_k - W_g.  ``check`` as in ``run_sel``."""
        M = (self.N if M is None else int(M)) if sel is None else int(sel.numel())
        self._topk_args('topk_threshold', W_all, W_g, e, kcount, tau, kept, ws, sel, M, check)
        _lib.check(_lib.lib().fs_topk_threshold(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                                self.len, _lib.ptr(W_g), _lib.ptr(e), int(kcount), _lib.ptr(tau),
                                                _lib.ptr(kept), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                                _lib.stream_ptr()), 'fs_topk_threshold')
        return tau, kept

    def run_topk(self, W_all, q, kcount, W_g, e, tau, kept, sel=None, ws=None, check=True):
        """fs_aggregate_topk: top-k sparsified uploads with error feedback over the rows ``sel`` of ``W_all``
        (None: rows 0..len(q)-1), in place with x = ``W_g`` on entry: a_k = (W_k - x) + e_k, kept where its
        magnitude key is at or above the row's ``kcount``-th largest (ties kept), ``W_g = x + sum_k
        q_k * kept(a_k)`` folded as ``run_opt`` folds its delta, and e_k = the part not kept (``e`` float32 with
        rows as ``W_all``, by client id; None: no memory).  ``tau`` float32 [M] (the threshold keys' bits) and
        ``kept`` int32 [M] are written.  The rule: include/fedsim.h.  ``check`` as in ``run_sel``."""
        M = int(q.numel())
        if not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()):
            raise ValueError('run_topk: q must be a contiguous float32 device tensor')
        self._topk_args('run_topk', W_all, W_g, e, kcount, tau, kept, ws, sel, M, check)
        _lib.check(_lib.lib().fs_aggregate_topk(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                                _lib.ptr(q), M, self.len, int(kcount), _lib.ptr(W_g), _lib.ptr(e),
                                                _lib.ptr(tau), _lib.ptr(kept), _lib.ptr(self.ws), self.ws.numel(),
                                                int(self.chunks), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                                _lib.stream_ptr()), 'fs_aggregate_topk')
        return W_g

    def dp_ws(self, M=None):
        """A uint8 workspace for ``run_dp`` / ``dp_norms`` at up to ``M`` rows (None: N): fs_aggregate_dp_ws_bytes
        (the norms and their partial table)."""
        return torch.empty(max(16, dp_ws_bytes(self.N if M is None else int(M), self.len)), dtype=torch.uint8,
                           device=self.ws.device)

    def _dp_rows(self, what, W_all, W_g, ws, sel, M, check):
        def ok(x, dt, cnt):
            return x is not None and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= cnt
        rows = W_all.numel() // self.len
        if not (M >= 1 and ok(W_all, torch.float32, self.len) and ok(W_g, torch.float32, self.len)
                and ok(ws, torch.uint8, dp_ws_bytes(M, self.len))):
            raise ValueError('%s: W_all, W_g (float32) and ws (uint8, dp_ws()) must be contiguous device tensors' % what)
        if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous()
                                    and sel.numel() == M):
            raise ValueError('%s: sel must be a contiguous int32 device tensor of M ids' % what)
        if sel is None and M > rows:
            raise ValueError('%s: W_all has fewer than M rows' % what)
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('%s: sel must index rows of W_all, [0, %d)' % (what, rows))

    @staticmethod
    def _dp_outs(what, M, c, r, state, q, clip_dev, adaptive):
        def ok(x, dt, cnt):
            return x is not None and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= cnt
        if not (ok(c, torch.float32, M) and ok(r, torch.float64, M) and ok(state, torch.float64, DP_STATE)
                and (q is None or (ok(q, torch.float32, M) and q.numel() == M))
                and (adaptive is None or ok(clip_dev, torch.float64, 1))):
            raise ValueError('%s: c (float32 [M]), r (float64 [M]), state (float64 [%d]), q (float32 [M] or None) and, '
                             'with adaptive, clip_dev (float64 [1]) must be contiguous device tensors'
                             % (what, DP_STATE))

    @staticmethod
    def _dp_rule(clip, noise_multiplier, seed, t, adaptive):
        ad = dict(adaptive or {})
        return (float(clip), float(noise_multiplier), int(seed), int(t), int(adaptive is not None),
                float(ad.get('quantile', 0.0)), float(ad.get('lr', 0.0)), float(ad.get('count_noise', 0.0)))

    def dp_norms(self, W_all, W_g, n, sel=None, M=None, ws=None, check=True):
        """fs_dp_norms: the squared norms of the updates ``W_all[row_k] - W_g`` of the rows ``sel`` (None: rows
        0..M-1, M = N unless given) into ``n`` float64 [M]: float squares summed in a fixed order, the same
        bits on every call.  ``check`` as in ``run_sel``."""
        M = (self.N if M is None else int(M)) if sel is None else int(sel.numel())
        ws = self.dp_ws(M) if ws is None else ws
        self._dp_rows('dp_norms', W_all, W_g, ws, sel, M, check)
        if not (n is not None and n.is_cuda and n.dtype == torch.float64 and n.is_contiguous() and n.numel() >= M):
            raise ValueError('dp_norms: n must be a contiguous float64 device tensor of M values')
        _lib.check(_lib.lib().fs_dp_norms(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                          self.len, _lib.ptr(W_g), _lib.ptr(n), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), 'fs_dp_norms')
        return n

    def dp_coef(self, n, q, clip, noise_multiplier, c, r, state, seed=0, t=0, adaptive=None, clip_dev=None):
        """fs_dp_coef: from the squared norms ``n`` float64 [M] and the weights ``q`` float32 [M] (None: 1 / M)
        the clip coefficients ``c`` float32 [M], the norms ``r`` float64 [M] and ``state`` float64 [DP_STATE] =
        (clip, sigma, b, dropped, clip_next).  ``adaptive``: dict(quantile, lr, count_noise); the clip is then
        read from and written back to ``clip_dev`` float64 [1]."""
        M = int(n.numel())
        if not (n.is_cuda and n.dtype == torch.float64 and n.is_contiguous()):
            raise ValueError('dp_coef: n must be a contiguous float64 device tensor')
        self._dp_outs('dp_coef', M, c, r, state, q, clip_dev, adaptive)
        S, z, seed, t, ad, ga, eta, sb = self._dp_rule(clip, noise_multiplier, seed, t, adaptive)
        _lib.check(_lib.lib().fs_dp_coef(_lib.ptr(n), _lib.ptr(q), M, S, z, seed, t, ad, ga, eta, sb,
                                         _lib.ptr(clip_dev) if ad else None, _lib.ptr(c), _lib.ptr(r),
                                         _lib.ptr(state), _lib.stream_ptr()), 'fs_dp_coef')
        return c, r, state

    def dp_noise(self, seed, t, g, stream=0):
        """fs_dp_noise: the Gaussian field of (``seed``, ``t``, ``stream``) into ``g`` float32 (a multiple of 4
        values): Philox4x32-10 at counter (i // 4, t, stream, 0), Box-Muller in double.  Stream 0 is the
        model noise of ``run_dp``."""
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise ValueError('dp_noise: g must be a contiguous float32 device tensor')
        _lib.check(_lib.lib().fs_dp_noise(int(seed), int(t), int(stream), g.numel(), _lib.ptr(g),
                                          _lib.stream_ptr()), 'fs_dp_noise')
        return g

    def run_dp(self, W_all, q, clip, noise_multiplier, W_g, c, r, state, seed=0, t=0, adaptive=None, clip_dev=None,
               sel=None, M=None, ws=None, check=True, cols=None):
        """fs_aggregate_dp: DP-FedAvg's server step over the rows ``sel`` of ``W_all`` (None: rows 0..M-1, M =
        len(q), or N with ``q`` None), in place with x = ``W_g`` on entry: every update W_k - x scaled to a norm
        of at most ``clip`` (rows with a non-finite norm dropped), folded with ``q`` (None: 1 / M) as ``run_opt``
        folds its delta, and ``noise_multiplier * clip * max q`` times the field of (``seed``, ``t``) added.
        ``c``, ``r``, ``state``, ``adaptive`` and ``clip_dev`` as in ``dp_coef``.  ``cols``: None, or (ld, D) for
        rows of ld floats of which the first D are parameters (the others take no noise).  The rule: include/fedsim.h.
        ``check`` as in ``run_sel``."""
        if sel is not None:
            M = int(sel.numel())
        elif q is not None:
            M = int(q.numel())
        else:
            M = self.N if M is None else int(M)
        ws = self.dp_ws(M) if ws is None else ws
        self._dp_rows('run_dp', W_all, W_g, ws, sel, M, check)
        self._dp_outs('run_dp', M, c, r, state, q, clip_dev, adaptive)
        S, z, seed, t, ad, ga, eta, sb = self._dp_rule(clip, noise_multiplier, seed, t, adaptive)
        _lib.check(_lib.lib().fs_aggregate_dp(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel),
                                              _lib.ptr(q), M, self.len, S, z, seed, t, ad, ga, eta, sb,
                                              _lib.ptr(clip_dev) if ad else None,
                                              0 if cols is None else int(cols[0]), 0 if cols is None else int(cols[1]),
                                              _lib.ptr(W_g), _lib.ptr(c),
                                              _lib.ptr(r), _lib.ptr(state), _lib.ptr(self.ws), self.ws.numel(),
                                              int(self.chunks), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   'fs_aggregate_dp')
        return W_g

    def run_robust(self, W_all, b, out, sel=None, check=True):
        """fs_aggregate_robust: the coordinate-wise trimmed mean of the rows ``sel`` of ``W_all`` (None:
        rows 0..N-1) with the trim count ``b``, 0 <= 2b < M: per coordinate the b smallest and the b
        largest values (by the total order of include/fedsim.h: -0 < +0, NaN at the ends) are
        dropped and the rest averaged in float64, rounded once.  ``b = 0``: the uniform mean;
        ``b = (M - 1) // 2``: the median.  ``out`` float32 [len], any buffer outside the selected rows.
        One launch; ``check`` as in ``run_sel``.  ValueError for M above ``robust_max_m()``."""
        M = self.N if sel is None else int(sel.numel())
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= self.len
                and W_all.is_cuda and W_all.dtype == torch.float32 and W_all.is_contiguous()):
            raise ValueError('run_robust: W_all and out must be contiguous float32 device tensors')
        if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and M >= 1):
            raise ValueError('run_robust: sel must be a contiguous, non-empty int32 device tensor')
        rows = W_all.numel() // self.len
        if sel is None and M > rows:
            raise ValueError('run_robust: W_all has fewer than N rows')
        if M > robust_max_m():
            raise ValueError('run_robust: M = %d is above fs_aggregate_robust_max_m() = %d' % (M, robust_max_m()))
        if check and sel is not None:
            lo, hi = int(sel.min().item()), int(sel.max().item())
            if lo < 0 or hi >= rows:
                raise ValueError('run_robust: sel must index rows of W_all, [0, %d)' % rows)
        _lib.check(_lib.lib().fs_aggregate_robust(_lib.ptr(W_all), self.len, None if sel is None else _lib.ptr(sel), M,
                                                  self.len, int(b), _lib.ptr(out), _lib.stream_ptr()),
                   'fs_aggregate_robust')
        return out


def topk_ws_bytes(M, length):
    """fs_aggregate_topk_ws_bytes: the bytes of workspace fs_aggregate_topk's select needs at M rows of
    ``length`` floats (0: it keeps its counts in LDS)."""
    return int(_lib.lib().fs_aggregate_topk_ws_bytes(int(M), int(length)))


DP_STATE = 5      # FS_DP_STATE: clip, sigma, b, dropped, clip_next


def dp_ws_bytes(M, length):
    """fs_aggregate_dp_ws_bytes: the bytes of workspace fs_aggregate_dp's norm pass needs at M rows of
    ``length`` floats (the norms and their partial table)."""
    return int(_lib.lib().fs_aggregate_dp_ws_bytes(int(M), int(length)))


RFA_INITS = {'start': 0, 'mean': 1}      # FS_RFA_INIT_*


def rfa_max_m():
    """fs_aggregate_rfa_max_m: the largest number of rows ``Aggregator.run_rfa`` accepts."""
    return int(_lib.lib().fs_aggregate_rfa_max_m())


def rfa_width(M):
    """fs_rfa_width: the columns of a stripe of fs_rfa_step at M rows (32, 16 or 8) -- it fixes the
    summation orders (include/fedsim.h)."""
    return int(_lib.lib().fs_rfa_width(int(M)))


def rfa_ws_bytes(M, length):
    """fs_aggregate_rfa_ws_bytes: the bytes of workspace fs_aggregate_rfa needs at up to M rows of
    ``length`` floats."""
    return int(_lib.lib().fs_aggregate_rfa_ws_bytes(int(M), int(length)))


def rfa_step(W_all, length, v, b, flag, v_out, part, sel=None, M=None):
    """fs_rfa_step: one iteration from one read of the rows ``sel`` of ``W_all`` (None: rows 0..M-1), each of
    ``length`` floats.  ``b`` / ``flag`` None: pass 0 (``v_out`` = ``v``); else ``v_out`` = the fold with the
    weights ``b`` float32 [M] (``flag`` int32 [1] non-zero: ``v`` instead).  ``part`` float64
    [ceil(length / rfa_width(M)), M] takes every row's partial squared distance to ``v_out`` per stripe."""
    M = int(sel.numel()) if sel is not None else int(M)
    W = max(1, rfa_width(M))
    for name, t, dt, n in (('W_all', W_all, torch.float32, 1 if sel is not None else M * int(length)),
                           ('v', v, torch.float32, int(length)), ('v_out', v_out, torch.float32, int(length)),
                           ('part', part, torch.float64, -(-int(length) // W) * M)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= n):
            raise ValueError('rfa_step: %s must be a contiguous %s device tensor of at least %d elements' % (name, dt, n))
    if (b is None) != (flag is None):
        raise ValueError('rfa_step: b and flag come together')
    if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() >= M
                              and flag.is_cuda and flag.dtype == torch.int32 and flag.numel() >= 1):
        raise ValueError('rfa_step: b (float32 [M]) and flag (int32 [1]) must be contiguous device tensors')
    if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous()):
        raise ValueError('rfa_step: sel must be a contiguous int32 device tensor')
    _lib.check(_lib.lib().fs_rfa_step(_lib.ptr(W_all), int(length), None if sel is None else _lib.ptr(sel), M,
                                      int(length), _lib.ptr(v), None if b is None else _lib.ptr(b),
                                      None if flag is None else _lib.ptr(flag), _lib.ptr(v_out), _lib.ptr(part),
                                      _lib.stream_ptr()), 'fs_rfa_step')
    return v_out, part


def rfa_weights(part, M, length, alpha, nu, d2, dist, b, obj, flag, mean=False):
    """fs_rfa_weights: ``part`` (``rfa_step``'s table; None: ``d2`` as given) reduced into ``d2`` float64 [M],
    then ``dist`` float64 [M], the weights ``b`` float32 [M], the objective ``obj`` float64 [1] and ``flag``
    int32 [1] (1: no finite row) under ``alpha`` float32 [M] and ``nu``; ``mean``: the weighted-mean weights."""
    M = int(M)
    for name, t, dt, n in (('alpha', alpha, torch.float32, M), ('d2', d2, torch.float64, M),
                           ('dist', dist, torch.float64, M), ('b', b, torch.float32, M),
                           ('obj', obj, torch.float64, 1), ('flag', flag, torch.int32, 1)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= n):
            raise ValueError('rfa_weights: %s must be a contiguous %s device tensor of at least %d elements'
                             % (name, dt, n))
    if part is not None and not (part.is_cuda and part.dtype == torch.float64 and part.is_contiguous()
                                 and part.numel() >= -(-int(length) // max(1, rfa_width(M))) * M):
        raise ValueError('rfa_weights: part must be a contiguous float64 device tensor [stripes, M]')
    _lib.check(_lib.lib().fs_rfa_weights(None if part is None else _lib.ptr(part), M, int(length), _lib.ptr(alpha),
                                         float(nu), int(bool(mean)), _lib.ptr(d2), _lib.ptr(dist), _lib.ptr(b),
                                         _lib.ptr(obj), _lib.ptr(flag), _lib.stream_ptr()), 'fs_rfa_weights')
    return b


def krum_max_m():
    """fs_aggregate_krum_max_m: the largest number of rows ``Aggregator.run_krum`` accepts."""
    return int(_lib.lib().fs_aggregate_krum_max_m())


def krum_split(M, length):
    """fs_krum_split: (slices of the len axis, K-steps of 32 elements per slice) of fs_krum_distances at
    M rows of ``length`` floats -- its summation order (include/fedsim.h)."""
    import ctypes
    s, k = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().fs_krum_split(int(M), int(length), ctypes.byref(s), ctypes.byref(k)), 'fs_krum_split')
    return s.value, k.value


def krum_select(D, M, f, m, score, pick, q=None, sel=None, rank=None):
    """fs_krum_select: from the float32 distance matrix ``D`` [M, krum_ldd(M)] alone, every row's score
    (float64 ``score`` [M]: the sum of its M - f - 2 smallest distances to the others) and the row ids of
    the ``m`` smallest (score, position) in ascending position (int32 ``pick`` [m]; ``sel`` int32 [M] maps
    positions to ids, None: the identity).  ``q`` float32 [m], if given, is set to f32(1 / m); ``rank``
    int32 [M] of scratch (None: allocated here), left holding every row's rank."""
    M, m = int(M), int(m)
    if rank is None:
        rank = torch.empty(max(1, M), dtype=torch.int32, device=D.device)
    if not (rank.is_cuda and rank.dtype == torch.int32 and rank.is_contiguous() and rank.numel() >= M):
        raise ValueError('krum_select: rank must be a contiguous int32 device tensor of M elements')
    if not (D.is_cuda and D.dtype == torch.float32 and D.is_contiguous() and D.numel() >= M * krum_ldd(M)
            and score.is_cuda and score.dtype == torch.float64 and score.is_contiguous() and score.numel() >= M
            and pick.is_cuda and pick.dtype == torch.int32 and pick.is_contiguous() and pick.numel() >= max(1, m)):
        raise ValueError('krum_select: D (float32 [M, ldD]), score (float64 [M]) and pick (int32 [m]) must be '
                         'contiguous device tensors')
    if q is not None and not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.numel() >= max(1, m)):
        raise ValueError('krum_select: q must be a contiguous float32 device tensor of m elements')
    if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() >= M):
        raise ValueError('krum_select: sel must be a contiguous int32 device tensor of M elements')
    _lib.check(_lib.lib().fs_krum_select(_lib.ptr(D), M, int(f), m, None if sel is None else _lib.ptr(sel),
                                         _lib.ptr(score), _lib.ptr(pick), None if q is None else _lib.ptr(q),
                                         _lib.ptr(rank), _lib.stream_ptr()), 'fs_krum_select')
    return score, pick


def krum_ldd(M):
    """The row pitch of fs_krum_distances' matrix: M rounded up to 4."""
    return (int(M) + 3) & ~3


def robust_max_m():
    """fs_aggregate_robust_max_m: the largest number of rows ``Aggregator.run_robust`` accepts."""
    return int(_lib.lib().fs_aggregate_robust_max_m())



def qffl_coef(F, p, q, L, u, g, sel=None):
    """fs_qffl_coef: the q-FedAvg coefficients of a round on the device, from the losses
    ``LocalEvaluator.run`` left in ``F`` [N, 2] float64: ``u_k = p_k Ft^q``, ``g_k = p_k q Ft^(q-1) L^2``
    with ``Ft = F[sel_k, 0] + 1e-10`` (``sel`` None: row k), computed in float64 and rounded once.
    ``p``, ``u``, ``g`` float32 device tensors of len(p) entries; ``sel`` int32 as long as ``p``."""
    M = int(p.numel())
    for x, dt in ((p, torch.float32), (u, torch.float32), (g, torch.float32)):
        if not (x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() >= M):
            raise ValueError('qffl_coef: p, u and g must be contiguous float32 device tensors of len(p) entries')
    if not (F.is_cuda and F.dtype == torch.float64 and F.is_contiguous()):
        raise ValueError('qffl_coef: F must be a contiguous float64 device tensor [N, 2]')
    if sel is not None and not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() >= M):
        raise ValueError('qffl_coef: sel must be a contiguous int32 device tensor as long as p')
    if sel is None and F.numel() < 2 * M:
        raise ValueError('qffl_coef: F has fewer rows than p has entries')
    _lib.check(_lib.lib().fs_qffl_coef(_lib.ptr(F), None if sel is None else _lib.ptr(sel), _lib.ptr(p), float(q),
                                       float(L), M, _lib.ptr(u), _lib.ptr(g), _lib.stream_ptr()), 'fs_qffl_coef')
    return u, g


class Evaluator:
    """fs_eval on a resident test set (``loss='mse'``: fs_eval_mse on float targets, C = 1)."""

    def __init__(self, X_test, y_test, D, C, device, ld=None, loss='ce'):
        if loss not in ('ce', 'mse'):
            raise ValueError("loss must be 'ce' or 'mse'")
        if loss == 'mse' and int(C) != 1:
            raise ValueError("loss='mse' needs C == 1")
        self.loss = loss
        self.f = Features([torch.as_tensor(X_test)], [torch.as_tensor(y_test)], D, device, ld,
                          float_targets=loss == 'mse')
        self.C = int(C)
        self.n = int(self.f.rows)
        if self.n < 1:
            raise ValueError('empty test set')
        self.ws = torch.empty(int(_lib.lib().fs_eval_ws_doubles(self.n)), dtype=torch.float64, device=device)

    def run(self, W, out2):
        if self.loss == 'mse':
            _lib.check(_lib.lib().fs_eval_mse(_lib.ptr(self.f.phi), self.f.ld, _lib.ptr(self.f.y), self.n, _lib.ptr(W),
                                              _lib.ptr(out2), _lib.ptr(self.ws), _lib.stream_ptr()), 'fs_eval_mse')
            return out2
        _lib.check(_lib.lib().fs_eval(_lib.ptr(self.f.phi), self.f.ld, _lib.ptr(self.f.labels), self.n, _lib.ptr(W),
                                      self.C, _lib.ptr(out2), _lib.ptr(self.ws), _lib.stream_ptr()), 'fs_eval')
        return out2


class ClientEvaluator:
    """Per-client evaluation (fs_z_eval_*): the (loss, accuracy %) of each of up to ``N`` client
    models on a resident row set, as one fs_mix_z GEMM per row chunk and one streaming reduction
    of its logits -- instead of N fs_eval calls that each read the features again.

    ``feats``: a ``Features`` with one row set, shared with its owner (an ``Evaluator``'s or a
    ``Mixture``'s ``.f``); labels, or float targets under ``loss='mse'`` (C = 1).  Owns the
    partial-sum workspace and a scratch Z for ``run``, allocated at its first call and bounded by
    ``scratch_bytes`` (``chunk_rows`` overrides the rows per chunk; rounded up to the row block).
    A client's result depends on its own model and the rows alone -- not on ``n_models``, its
    position or the chunking (bitwise; include/fedsim.h)."""

    def __init__(self, feats, C, N, loss='ce', scratch_bytes=256 << 20, chunk_rows=None):
        if loss not in ('ce', 'mse'):
            raise ValueError("loss must be 'ce' or 'mse'")
        if loss == 'mse' and (int(C) != 1 or feats.y is None):
            raise ValueError("loss='mse' needs C == 1 and Features(float_targets=True)")
        if loss == 'ce' and feats.labels is None:
            raise ValueError("loss='ce' needs integer labels")
        self.loss, self.f, self.C, self.N = loss, feats, int(C), int(N)
        self.n = int(feats.rows)
        if self.n < 1 or self.N < 1:
            raise ValueError('ClientEvaluator needs at least one row and one model')
        L = _lib.lib()
        self.block = int(L.fs_z_eval_block_rows())
        self.ws = torch.empty(int(L.fs_z_eval_ws_doubles(self.n, self.N)), dtype=torch.float64, device=feats.device)
        ldN = (self.N + 3) // 4 * 4
        if chunk_rows:
            blocks = (int(chunk_rows) + self.block - 1) // self.block
        else:
            blocks = int(scratch_bytes) // (4 * self.C * ldN) // self.block
        self.chunk_rows = self.block * max(1, min(blocks, (self.n + self.block - 1) // self.block))
        self.Z = None

    def _add(self, Z, row0, rows, n_models):
        L = _lib.lib()
        if self.loss == 'mse':
            _lib.check(L.fs_z_eval_add_mse(_lib.ptr(Z), _lib.ptr(self.f.y), self.n, int(row0), int(rows),
                                           int(n_models), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                       'fs_z_eval_add_mse')
        else:
            _lib.check(L.fs_z_eval_add(_lib.ptr(Z), _lib.ptr(self.f.labels), self.n, int(row0), int(rows),
                                       int(n_models), self.C, _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                       'fs_z_eval_add')

    def _finish(self, n_models, out):
        if not (out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= 2 * int(n_models)):
            raise ValueError('out must be a contiguous float64 tensor of [n_models, 2]')
        _lib.check(_lib.lib().fs_z_eval_finish(_lib.ptr(self.ws), self.ws.numel(), self.n, int(n_models),
                                               _lib.ptr(out), _lib.stream_ptr()), 'fs_z_eval_finish')
        return out

    def _check_models(self, n_models):
        if not 1 <= int(n_models) <= self.N:
            raise ValueError('n_models must be in [1, %d]' % self.N)

    def run(self, W_all, n_models, out):
        """``W_all`` [>= n_models, C, ld]: fs_mix_z on row chunks of the features, each reduced by
        fs_z_eval_add; ``out`` [n_models, 2] float64 (loss, accuracy %).  Current stream."""
        self._check_models(n_models)
        ldN = (int(n_models) + 3) // 4 * 4
        if self.Z is None:
            self.Z = torch.empty(self.chunk_rows * self.C * ((self.N + 3) // 4 * 4), dtype=torch.float32,
                                 device=self.f.device)
        f, L = self.f, _lib.lib()
        assert self.chunk_rows * self.C * ldN <= self.Z.numel()
        for row0 in range(0, self.n, self.chunk_rows):
            rows = min(self.chunk_rows, self.n - row0)
            _lib.check(L.fs_mix_z(_lib.ptr(W_all), _lib.ptr(f.phi[row0:]), f.ld, int(n_models), self.C, rows,
                                  _lib.ptr(self.Z), _lib.stream_ptr()), 'fs_mix_z')
            self._add(self.Z, row0, rows, n_models)
        return self._finish(n_models, out)

    def run_z(self, Z, n_models, out):
        """The reduction alone, on logits that already exist: ``Z`` [n, C * ldN(n_models)] in
        fs_mix_z's layout on this evaluator's rows (FedAMW: the p-solve's Z)."""
        self._check_models(n_models)
        ldN = (int(n_models) + 3) // 4 * 4
        if Z.dtype != torch.float32 or not Z.is_contiguous() or Z.numel() < self.n * self.C * ldN:
            raise ValueError('Z must be a contiguous float32 tensor of [n, C * ldN]')
        self._add(Z, 0, self.n, n_models)
        return self._finish(n_models, out)


class LocalEvaluator:
    """Local evaluation (fs_eval_clients): the (loss, accuracy %) of a model on every client's
    OWN rows of a resident training ``Features`` (shared with its owner, a ``LocalTrainer``'s
    ``.f``), one pass over the features instead of N fs_eval calls on row slices.

    ``run(W, stride, out)``: client j's model is ``W`` + j * ``stride`` floats -- stride 0 scores
    one model (the global one) on every client, stride C * ld the clients x params buffer
    (``W_out[j]`` on client j).  Owns the workspace.  A client's two numbers are bitwise what
    ``Evaluator.run`` gives on its row slice (include/fedsim.h, contract A)."""

    def __init__(self, feats, C, loss='ce'):
        if loss not in ('ce', 'mse'):
            raise ValueError("loss must be 'ce' or 'mse'")
        if loss == 'mse' and (int(C) != 1 or feats.y is None):
            raise ValueError("loss='mse' needs C == 1 and Features(float_targets=True)")
        if loss == 'ce' and feats.labels is None:
            raise ValueError("loss='ce' needs integer labels")
        self.loss, self.f, self.C = loss, feats, int(C)
        self.N = int(len(feats.ns))
        if self.N < 1 or int(feats.ns.min()) < 1:
            raise ValueError('LocalEvaluator needs at least one client and one row per client')
        self._h_n = np.ascontiguousarray(feats.ns, dtype=np.int64)
        self.ws = torch.empty(int(_lib.lib().fs_eval_clients_ws_doubles(int(feats.rows), self.N)),
                              dtype=torch.float64, device=feats.device)

    def run(self, W, stride, out):
        """``out`` [N, 2] float64 (loss, accuracy %) on the current stream."""
        stride = int(stride)
        need = (self.N - 1) * stride + self.C * self.f.ld
        if W.dtype != torch.float32 or not W.is_contiguous() or W.numel() < need:
            raise ValueError('W must be a contiguous float32 tensor of at least %d floats' % need)
        if not (out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= 2 * self.N):
            raise ValueError('out must be a contiguous float64 tensor of [N, 2]')
        f, L = self.f, _lib.lib()
        if self.loss == 'mse':
            _lib.check(L.fs_eval_clients_mse(_lib.ptr(f.phi), f.ld, _lib.ptr(f.row_off_dev), self._h_n.ctypes.data,
                                             _lib.ptr(f.y), self.N, _lib.ptr(W), stride, _lib.ptr(out),
                                             _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                       'fs_eval_clients_mse')
        else:
            _lib.check(L.fs_eval_clients(_lib.ptr(f.phi), f.ld, _lib.ptr(f.row_off_dev), self._h_n.ctypes.data,
                                         _lib.ptr(f.labels), self.N, _lib.ptr(W), stride, self.C, _lib.ptr(out),
                                         _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                       'fs_eval_clients')
        return out


class Mixture:
    """FedAMW's mixture-weight estimation: Z GEMM + persistent p-SGD (tools.py:435-453).
    ``loss='mse'``: float validation targets, C = 1, fs_mix_solve_mse (one workgroup; the
    rank-blocked Z layout is never asked for)."""

    def __init__(self, X_val, y_val, D, C, N, Bv, p0, device, ld=None, momentum=0.9, loss='ce'):
        if loss not in ('ce', 'mse'):
            raise ValueError("loss must be 'ce' or 'mse'")
        if loss == 'mse' and int(C) != 1:
            raise ValueError("loss='mse' needs C == 1")
        self.loss = loss
        self.f = Features([torch.as_tensor(X_val)], [torch.as_tensor(y_val)], D, device, ld,
                          float_targets=loss == 'mse')
        self.C, self.N, self.Bv = int(C), int(N), int(Bv)
        self.nv = int(self.f.rows)
        if self.nv < 1:
            raise ValueError('empty validation set')
        self.momentum = float(momentum)
        self.ldN = (self.N + 3) // 4 * 4
        self.Z = torch.empty(self.nv, self.C * self.ldN, dtype=torch.float32, device=device)
        self.p = p0.to(device=device, dtype=torch.float32).clone()
        self.buf = torch.zeros(self.N, dtype=torch.float32, device=device)
        self.first = torch.ones(1, dtype=torch.int32, device=device)
        self.ws = torch.zeros(int(_lib.lib().fs_mix_solve_ws_bytes(self.N, self.C, self.Bv)), dtype=torch.uint8,
                              device=device)
        self.shuffler = None
        self.blocks = 1          # > 1: Z holds `blocks` rank blocks [blocks][n_val][C][N/blocks] (dist.py)

    def blocked_covers(self, epochs):
        """Whether fs_mix_solve_blocked reads this shape (the qmc solver; include/fedsim.h).
        Never under loss='mse'."""
        if self.loss == 'mse':
            return False
        return bool(_lib.lib().fs_mix_solve_blocked_covers(self.N, self.C, self.nv, int(epochs), self.Bv))

    def check_errors(self):
        """Raise if a multi-CU p-solve reported a timed-out exchange (synchronises)."""
        _check_ws_error(self.ws, 'fs_mix_solve')

    def z_block(self, W_all, n, out):
        """fs_mix_z of ``n`` client models (W_all [n, C, ld]) on the validation rows into
        ``out`` [n_val, C * ldN(n)] -- one rank's block of the sharded Z-GEMM."""
        _lib.check(_lib.lib().fs_mix_z(_lib.ptr(W_all), _lib.ptr(self.f.phi), self.f.ld, int(n), self.C, self.nv,
                                       _lib.ptr(out), _lib.stream_ptr()), 'fs_mix_z')
        return out

    def prepare(self, seeds, slot=0, stream=None):
        """Enqueue one round's validation-pass shuffles (one seed per inner epoch)."""
        ep = len(seeds)
        if self.shuffler is None or self.shuffler.P != ep:
            self.shuffler = Shuffler(np.full(ep, self.nv, np.int64), np.arange(ep, dtype=np.int64) * self.nv,
                                     ep * self.nv, self.Z.device)
        self.shuffler.prepare(seeds, slot, stream)

    def solve(self, W_all, seeds, lr_p, slot=None, z=True):
        """W_all: [N, C, ld] every client's weights; seeds: sampler seeds of the round's
        validation passes (one per inner epoch), or None when ``prepare`` already enqueued
        them into ``slot``.  ``z=False`` reuses Z from the previous call (W_all unchanged)."""
        L = _lib.lib()
        if z and self.blocks > 1:
            # fs_mix_z writes the standard [n_val][C][ldN] layout; fs_mix_solve_blocked would
            # read it as rank blocks
            raise ValueError('Mixture.solve(z=True) with blocks=%d: Z must come from the rank-block '
                             'all-gather (dist.allgather_z(blocked=True)), then solve(z=False)' % self.blocks)
        if z:
            _lib.check(L.fs_mix_z(_lib.ptr(W_all), _lib.ptr(self.f.phi), self.f.ld, self.N, self.C, self.nv,
                                  _lib.ptr(self.Z), _lib.stream_ptr()), 'fs_mix_z')
        if seeds is not None:
            slot = 0
            if len(seeds) == 0:
                return self.p
            self.prepare(seeds, slot)
        epochs = self.shuffler.P
        perms = self.shuffler.acquire(slot)
        if self.loss == 'mse':
            _lib.check(L.fs_mix_solve_mse(_lib.ptr(self.Z), _lib.ptr(self.f.y), _lib.ptr(perms), self.N, self.nv, epochs,
                                          self.Bv, float(lr_p), self.momentum, _lib.ptr(self.p), _lib.ptr(self.buf),
                                          _lib.ptr(self.first), _lib.ptr(self.ws), self.ws.numel(),
                                          _lib.stream_ptr()), 'fs_mix_solve_mse')
            self.shuffler.release(slot)
            return self.p
        tail = (_lib.ptr(self.f.labels), _lib.ptr(perms), self.N, self.C, self.nv, epochs, self.Bv, float(lr_p),
                self.momentum, _lib.ptr(self.p), _lib.ptr(self.buf), _lib.ptr(self.first), _lib.ptr(self.ws),
                self.ws.numel(), _lib.stream_ptr())
        if self.blocks > 1:
            _lib.check(L.fs_mix_solve_blocked(_lib.ptr(self.Z), self.blocks, *tail), 'fs_mix_solve_blocked')
        else:
            _lib.check(L.fs_mix_solve(_lib.ptr(self.Z), *tail), 'fs_mix_solve')
        self.shuffler.release(slot)
        return self.p


def feature_map(X, W, b, D, out=None, ldo=None):
    """fs_feature_map: ``scale * cos(X W + b)`` (tools.py:27, 29) on the current stream.
    X [n, d] (any device; copied to the GPU as fp32 if needed), W [d, D], b [D] -> out [n, ldo]
    (default ldo = D; columns D..ldo-1 are written as 0)."""
    dev = torch.device('cuda', torch.cuda.current_device())
    X = torch.as_tensor(X).to(device=dev, dtype=torch.float32).contiguous()
    W = torch.as_tensor(W).to(device=dev, dtype=torch.float32).reshape(-1, int(D)).contiguous()
    b = torch.as_tensor(b).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    n, d = X.shape
    if W.shape[0] != d or b.numel() != D:
        raise ValueError('feature_map: X [n, %d] needs W [%d, %d] and b [%d]' % (d, d, D, D))
    ldo = int(ldo or D)
    if out is None:
        out = torch.empty(n, ldo, device=dev, dtype=torch.float32)
    assert out.is_contiguous() and out.shape[1] == ldo and out.shape[0] >= n
    scale = float(np.float32(1.0 / np.sqrt(D)))      # the float64 scalar torch multiplies in fp32
    _lib.check(_lib.lib().fs_feature_map(_lib.ptr(X), d, _lib.ptr(W), _lib.ptr(b), n, d, int(D), scale,
                                         _lib.ptr(out), ldo, _lib.stream_ptr()), 'fs_feature_map')
    return out


def heterogeneity(feats):
    """exp.py:67-74 over a client-packed feature buffer (``Features``): fs_gram for
    G = Phi^T Phi, fs_hetero for S_j = ||G/n - G_j/n_j||_F^2 per client.  Returns
    (sum_j n_j/n * sqrt(S_j), S [N] numpy float64)."""
    dev = feats.phi.device
    D, N, n = feats.D, len(feats.ns), int(feats.rows)
    if n < 1:
        raise ValueError('heterogeneity of an empty partition')
    G = torch.empty(D, D, device=dev, dtype=torch.float32)
    S = torch.empty(N, device=dev, dtype=torch.float64)
    L = _lib.lib()
    _lib.check(L.fs_gram(_lib.ptr(feats.phi), feats.ld, n, D, _lib.ptr(G), D, _lib.stream_ptr()), 'fs_gram')
    _lib.check(L.fs_hetero(_lib.ptr(feats.phi), feats.ld, _lib.ptr(feats.row_off_dev), N, D, _lib.ptr(G), D, n,
                           _lib.ptr(S), _lib.stream_ptr()), 'fs_hetero')
    S = S.cpu().numpy()
    hete = np.float32(0.0)
    for nj, s in zip(feats.ns, S):      # data_hete += len_j / len * torch.norm(C - C_j), an fp32 tensor
        hete = np.float32(hete + np.float32(nj / n * np.float32(np.sqrt(s))))
    return float(hete), S
