"""Drop-in FedAvg / FedProx / FedNova / FedAMW (and SCAFFOLD) on MI355X.

Same names, positional signatures, defaults and return values as the reference
(/root/reference/functions/tools.py:329, 356, 383, 413):

    train_loss, test_loss, test_acc = FedAvg(X_train, y_train, X_test, y_test, type,
                                             num_classes, D, lr, epoch, batch_size, prox,
                                             mu, lambda_reg_if, lambda_reg, round)

* ``X_train`` / ``y_train``: per-client lists of feature matrices [n_j, D] (fp32) and
  integer labels (``type='regression'``: float targets of shape [n_j, 1]), on CPU or GPU;
  ``X_test`` / ``y_test`` likewise; FedAMW takes the
  reference's ``validloader`` (a DataLoader over a TensorDataset, batch 16, shuffle).
* Returns three CPU float32 tensors of length ``round``; ``test_acc`` is in percent.
  One ``Test loss: ..., \\t Test Acc: ...`` line per round is printed (tools.py:236),
  after the last round (the run is not synchronised per round).
* The global torch CPU generator is consumed exactly as the reference consumes it
  (MLP init, every DataLoader pass), so seeds and shuffles line up draw for draw.

Keyword-only extensions (not in the reference):
* ``clients='sequential'`` (default) -- the reference's semantics: the clients of a
  round are chained (client i starts from client i-1's trained weights and its
  FedProx anchor is that start); runs as one workgroup walking the chain.
  ``clients='parallel'`` -- every client starts from the round's global model (and is
  anchored to it); clients train concurrently, one workgroup each, and shard across
  GPUs when a torch.distributed process group is initialised.
* ``stats`` -- a dict that receives the final global model (and, with
  ``stats={'trace': True}``, the global model after every round in ``'W_rounds'``).
  ``stats={'client_eval': 'test'}`` (or ``'val'``, or ``('test', 'val')``) also scores EVERY
  client's local model each round, right after local training (chained clients: the chain's
  state after client j, the reference's ``local_weights[j]``): ``stats['client_test_loss']`` /
  ``['client_test_acc']`` and / or the ``client_val_*`` pair, CPU float64 tensors [round, N] in
  the caller's client order ([N] from Distributed and FedAMW_OneShot; Centralized has one model
  and ignores the key).  ``'val'`` scores on the validloader's rows, so it needs FedAMW or
  FedAMW_OneShot (ValueError otherwise), where it reuses the p-solve's logits.  One GEMM and one
  streaming reduction per round (engine.ClientEvaluator, fs_z_eval_*); without the key nothing
  is launched or allocated, and no generator is touched either way.
  ``stats={'local_eval': 'global'}`` (or ``'own'``, or ``('global', 'own')``) scores models on
  every client's OWN training rows each round (engine.LocalEvaluator, fs_eval_clients: one pass
  over the resident features).  ``'global'``: the round's aggregated model (FedAMW: the
  p-weighted one; the model ``test_loss[t]`` scores) on each client ->
  ``stats['local_global_loss']`` / ``['local_global_acc']``, and the true objective
  ``stats['global_objective']`` = sum_j (n_j / n) local_global_loss[:, j] (float64, client
  order) -- which ``train_loss`` is not: that is a running mean over the last local epoch, taken
  while the weights move, with the prox and ridge terms.  ``'own'``: each client's own trained
  model, right after local training (the reference's dropped ``train_acc.avg``,
  tools.py:213-215, but of the finished model) -> ``stats['local_own_loss']`` /
  ``['local_own_acc']``.  CPU float64 tensors [round, N] in the caller's client order
  (Distributed: [N]; FedAMW_OneShot: 'global' [round, N], 'own' [N]); Centralized pools the
  clients into one and raises a ValueError.  Nothing is drawn from any generator and the
  returns are bitwise those of the run without the key.

* ``participation`` / ``sample_seed`` (FedAvg, FedProx, FedNova, Scaffold; needs ``clients='parallel'``) -- partial
  client participation: only a sampled subset S_t of the clients trains in round t and is
  aggregated, ``W_g = sum_{j in S_t} q_j W_j`` with ``q = n[S_t] / sum(n[S_t])`` folded in ascending
  client id (fs_aggregate_sel reads the sampled rows only).  A float in (0, 1] is McMahan's
  fraction C (``M = max(1, floor(C N + 0.5))`` clients per round), an int in [1, N] is M itself, a
  sequence of ``round`` id arrays an explicit schedule (``functions/participation.py``).  The sampler
  is a private generator seeded with ``sample_seed``; only the sampled clients' DataLoader passes
  draw from the global generator (ascending client id, epoch-minor, then the test pass), as a
  loop over the sampled clients would.  ``train_loss[t] = sum(q * losses_S)``; evaluation, the lr
  schedule and the returns are as without the keyword, and ``participation=1.0`` is bitwise the
  call without it.  ``stats['participants']``: the R id arrays.  Unsampled clients of a round:
  NaN in ``stats['client_*']`` and ``stats['local_own_*']`` (``local_global_*`` covers all N).
  FedAMW and the single-shot algorithms take no such keyword (what p means over a changing
  subset is an open algorithm question).
* ``variant`` (FedNova) -- ``'reference'`` (default): the reference's aggregate, tools.py:401-405,
  bitwise its fold (fs_aggregate_nova mode 1); ``'updates'``: Wang et al.'s normalised averaging
  of the clients' updates (mode 2; needs ``clients='parallel'``).  See ``FedNova`` and DESIGN 4.2.2.

* ``Scaffold`` (not in the reference) -- SCAFFOLD with control variates, FedAvg's positional list,
  parallel clients; keyword-only ``server_lr``, ``weighting``, ``participation`` / ``sample_seed``
  (see ``Scaffold`` and DESIGN 4.1 / 4.2.3).

All arithmetic of the round runs in the gfx950 kernels of libfedsim.so; there is no
CPU path.

``type='classification'`` selects cross-entropy, ``type='regression'`` the reference's
``nn.MSELoss(reduction='mean')`` branch (tools.py:181-184, 221-224, 297-300, 419-422) at
``num_classes = 1`` (the reference's regression loader, utils.py:121, 167) with float targets
of shape [n, 1] (utils.py:81-82): fs_local_train_mse / fs_eval_mse / fs_mix_solve_mse.
``test_acc`` is then the reference's degenerate value, 100 * #{y_test == 0} / n
(comp_accuracy's top-1 index of a one-column output is always 0).  1-D float targets -- which
the reference broadcasts into a [B, B] loss -- are rejected with a ValueError, as are integer
or non-finite targets; ``num_classes != 1`` raises NotImplementedError, any other ``type`` a
ValueError.  ``stats['W_global']`` is [1, D] and ``stats['W_rounds']`` [R, 1, D].
"""

import math

import numpy as np
import torch

from .. import dist, engine, rng
from .. import _lib
from . import participation as _participation
from .._lib import FedsimError

__all__ = ['FedAvg', 'FedProx', 'FedNova', 'Scaffold', 'FedAMW', 'Centralized', 'Distributed', 'FedAMW_OneShot', 'Federation', 'RFF',
           'feature_mapping', 'update_learning_rate', 'init_weights']


def update_learning_rate(epoch, target_lr, T):
    """tools.py:43-61 (callers rebind lr, so the decay compounds: lr0, lr0/10, lr0/1000)."""
    if epoch == int(T / 2):
        return target_lr / 10
    if epoch == int(T * 0.75):
        return target_lr / 100
    return target_lr


def init_weights(D, C):
    """MLP(D, C) initialisation (tools.py:34-40): nn.Linear's Kaiming-uniform draw
    (discarded) then xavier_uniform_, on the global CPU generator -> [C, D] fp32."""
    w = torch.empty(C, D)
    torch.nn.init.kaiming_uniform_(w, a=5 ** 0.5)
    torch.nn.init.xavier_uniform_(w)
    return w


def _device():
    if not torch.cuda.is_available():
        raise FedsimError('fedamw_amd needs a ROCm GPU (MI355X); there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _check_labels(ys, num_classes, what):
    """Every label in [0, num_classes): the kernels index class rows by label, and the
    reference's CrossEntropyLoss raises on an out-of-range target."""
    for y in ys:
        y = torch.as_tensor(y)
        if y.numel() and (int(y.min()) < 0 or int(y.max()) >= num_classes):
            raise ValueError('%s labels must lie in [0, %d), got [%d, %d]' % (what, num_classes, int(y.min()),
                                                                              int(y.max())))


def _check_targets(ys, what):
    """Regression targets: float [n, 1], finite.  The reference's MSELoss broadcasts a [B, 1]
    output against 1-D [B] targets into a [B, B] loss (torch warns; every row then regresses
    onto the batch mean) -- not reproduced."""
    for y in ys:
        y = torch.as_tensor(y)
        if not y.dtype.is_floating_point:
            raise ValueError("%s targets must be floating point for type='regression', got %s" % (what, y.dtype))
        if y.dim() == 1:
            raise ValueError("%s targets are 1-D: the reference's MSELoss would broadcast its [B, 1] output against "
                             "[B] targets into a [B, B] loss; pass y.reshape(-1, 1)" % what)
        if y.dim() != 2 or y.shape[1] != 1:
            raise ValueError('%s targets must have shape [n, 1], got %s' % (what, tuple(y.shape)))
        if y.numel() and not bool(torch.isfinite(y).all()):
            raise ValueError('%s targets must be finite' % what)


def _loss_of(type):
    return 'mse' if type == 'regression' else 'ce'


def _check_inputs(type, X_train, y_train, num_classes, batch_size, epoch, round, y_test=None, y_val=None,
                  train_labels=True):
    if type not in ('classification', 'regression'):
        raise ValueError("type must be 'classification' or 'regression', got %r" % (type,))
    if type == 'regression' and int(num_classes) != 1:
        raise NotImplementedError("type='regression' is implemented for num_classes == 1 (the reference's "
                                  "regression loader, utils.py:121, 167); multi-output regression is out of scope")
    if len(X_train) != len(y_train) or len(y_train) == 0:
        raise ValueError('X_train and y_train must be equal-length non-empty lists')
    for y in y_train:
        if len(y) == 0:
            # torch.utils.data.RandomSampler rejects an empty dataset (raised inside train_loop)
            raise ValueError('num_samples should be a positive integer value, but got num_samples=0')
    if not (1 <= num_classes <= 32):
        raise NotImplementedError('num_classes must be in [1, 32]')
    if batch_size < 1:
        raise NotImplementedError('batch_size must be >= 1')
    if type == 'regression' and batch_size > 64:
        raise NotImplementedError("batch_size must be in [1, 64] for type='regression' (the MSE kernels have no "
                                  "batch-tiled form; classification takes any batch_size)")
    if epoch < 1 or round < 0:
        raise ValueError('epoch must be >= 1 and round >= 0')
    if type == 'regression':
        # (every client's targets, whatever train_labels says: shapes are checked before any device is touched)
        _check_targets(y_train, 'training')
        if y_test is not None:
            _check_targets([y_test], 'test')
        if y_val is not None:
            _check_targets([y_val], 'validation')
        return
    if train_labels:
        _check_labels(y_train, num_classes, 'training')
    if y_test is not None:
        _check_labels([y_test], num_classes, 'test')
    if y_val is not None:
        _check_labels([y_val], num_classes, 'validation')


def _client_eval_request(stats, has_val):
    """``stats['client_eval']``: 'test', 'val' or a tuple of both -> the row sets to score every
    client model on (() without the key).  'val' needs a validation set (FedAMW, FedAMW_OneShot)."""
    req = None if stats is None else stats.get('client_eval')
    if req is None:
        return ()
    req = (req,) if isinstance(req, str) else tuple(req)
    for r in req:
        if r not in ('test', 'val'):
            raise ValueError("stats['client_eval'] must be 'test', 'val' or ('test', 'val'), got %r" % (r,))
    if 'val' in req and not has_val:
        raise ValueError("stats['client_eval'] = 'val' needs a validloader (FedAMW, FedAMW_OneShot)")
    return tuple(dict.fromkeys(req))


def _client_eval_stats(stats, which, hist):
    """hist [..., N, 2] float64 (any device) -> stats['client_<which>_loss'] / ['client_<which>_acc']."""
    hist = hist.detach().cpu()
    stats['client_%s_loss' % which] = hist[..., 0].contiguous()
    stats['client_%s_acc' % which] = hist[..., 1].contiguous()


def _client_eval_once(stats, which, feats, C, N, task, W_out, Z=None):
    """One set of N local models (Distributed, FedAMW_OneShot) scored on one row set into ``stats``."""
    ce = engine.ClientEvaluator(feats, C, N, loss=task)
    out = torch.empty(N, 2, dtype=torch.float64, device=feats.device)
    if Z is not None:
        ce.run_z(Z, N, out)
    else:
        ce.run(W_out, N, out)
    _client_eval_stats(stats, which, out)


def _local_eval_request(stats):
    """``stats['local_eval']``: 'global', 'own' or a tuple of both -> the model sets to score on
    every client's own rows (() without the key)."""
    req = None if stats is None else stats.get('local_eval')
    if req is None:
        return ()
    req = (req,) if isinstance(req, str) else tuple(req)
    for r in req:
        if r not in ('global', 'own'):
            raise ValueError("stats['local_eval'] must be 'global', 'own' or ('global', 'own'), got %r" % (r,))
    return tuple(dict.fromkeys(req))


def _local_eval_stats(stats, which, hist, ns):
    """hist [..., N, 2] float64 (any device, the caller's client order) -> stats['local_<which>_loss']
    / ['local_<which>_acc']; 'global' also gives stats['global_objective'], the n_j-weighted sum
    of the losses in float64, client by client."""
    hist = hist.detach().cpu()
    loss = stats['local_%s_loss' % which] = hist[..., 0].contiguous()
    stats['local_%s_acc' % which] = hist[..., 1].contiguous()
    if which == 'global':
        w = np.asarray(ns, dtype=np.float64) / float(np.sum(ns))
        obj = torch.zeros(loss.shape[:-1], dtype=torch.float64)
        for j in range(loss.shape[-1]):
            obj += float(w[j]) * loss[..., j]
        stats['global_objective'] = obj


def _local_eval_once(stats, which, le, W, stride):
    """One model set scored once on every client's own rows (Distributed, FedAMW_OneShot 'own')."""
    out = torch.empty(le.N, 2, dtype=torch.float64, device=le.f.device)
    le.run(W, stride, out)
    _local_eval_stats(stats, which, out, le.f.ns)


# scheduling options of a Federation (how the launches of the rounds are arranged; none of
# them changes a result bit):
#   shuffle_chunk   FedAvg / FedProx with device-replayed shuffles: the shuffles of this many
#                   rounds come from one launch, one chunk ahead (1 = per round)
#   defer_eval      round t's test evaluation rides on round t+1's training launch where that
#                   launch leaves CUs idle (FS_PHASE_EVAL_DEFER)
#   fedamw_shuffle  'early': FedAMW's round t+1 shuffles run beside the Z GEMM; 'late': after
#                   the round, beside the p-solve
OPTIONS = {'shuffle_chunk': 8, 'defer_eval': True, 'fedamw_shuffle': 'early'}


NOVA_VARIANTS = ('reference', 'updates')


def _check_nova(variant, clients):
    """FedNova's keyword checks (host only: before any device is touched)."""
    if variant not in NOVA_VARIANTS:
        raise ValueError("variant must be 'reference' or 'updates'")
    if variant == 'updates' and clients != 'parallel':
        raise ValueError("variant='updates' needs clients='parallel': a chained client's W_j - W_g contains its "
                         "predecessors' work")


def nova_reference_coefficients(ns, epoch, batch_size):
    """The host scalars of tools.py:387-389 / 403-405 over the clients ``ns`` (all of them, or a
    round's sample in ascending id), by the reference's own torch expressions: p float32,
    Tau = n*E/B float64, Tau_eff = sum(Tau*p) float64; the weights tensors are float32, so
    line 403's factor reaches them as s0 = f32(f64(p_0)*Tau_eff/Tau_0) and line 405's as
    te = f32(Tau_eff), b_j = f32(Tau_j).  Returns (p, b, te, s0)."""
    ns = np.asarray(ns)
    p = torch.tensor(ns / sum(ns), dtype=torch.float32)
    Tau = torch.tensor(ns * epoch / batch_size)
    Tau_eff = torch.sum(Tau * p)
    s0 = (p[0] * Tau_eff / Tau[0]).to(torch.float32)
    return p, Tau.to(torch.float32), float(Tau_eff.to(torch.float32)), float(s0)


def nova_update_coefficients(ns, epoch, batch_size):
    """Wang et al.'s normalised averaging over the clients ``ns``: tau_j = E*ceil(n_j/B), the steps
    train_loop takes; tau_eff = sum_j p_j tau_j (float64, p float32 as tools.py:387);
    a_j = f32(p_j*tau_eff/tau_j), which sum to 1 up to rounding.  Returns (p, a)."""
    ns = np.asarray(ns)
    p = torch.tensor(ns / sum(ns), dtype=torch.float32)
    tau = torch.tensor(epoch * -(-ns // batch_size), dtype=torch.float64)
    tau_eff = torch.sum(p.to(torch.float64) * tau)
    return p, (p.to(torch.float64) * tau_eff / tau).to(torch.float32)


SCAFFOLD_WEIGHTINGS = ('size', 'uniform')


def _check_scaffold(type, prox, batch_size, weighting, server_lr):
    """Scaffold's keyword checks (host only: before any device is touched)."""
    if type != 'classification':
        raise ValueError("Scaffold is implemented for type='classification' (cross-entropy) only")
    if prox:
        raise ValueError('the prox term is not supported together with SCAFFOLD (prox=False)')
    if int(batch_size) > 64:
        raise ValueError('Scaffold needs batch_size <= 64 (the variate kernel has no batch-tiled form)')
    if weighting not in SCAFFOLD_WEIGHTINGS:
        raise ValueError("weighting must be 'size' or 'uniform'")
    if not float(server_lr) > 0.0:
        raise ValueError('server_lr must be > 0')


def scaffold_lr_schedule(lr, R):
    """The learning rate of every round: ``update_learning_rate`` compounded as the round loop
    rebinds it (lr0, lr0/10, lr0/1000)."""
    out = []
    for t in range(int(R)):
        lr = update_learning_rate(t, lr, R)
        out.append(lr)
    return out


def scaffold_weights(ns, weighting='size'):
    """The clients' global weights p (float64): n_i / n ('size') or 1 / N ('uniform')."""
    ns = np.asarray(ns, dtype=np.float64)
    if weighting == 'uniform':
        return np.full(len(ns), 1.0 / len(ns))
    return ns / float(np.sum(ns))


def scaffold_round_coefficients(ns, S, epoch, batch_size, lr, server_lr=1.0, weighting='size'):
    """SCAFFOLD's host scalars of one round with the sample ``S`` (ascending ids) at the round's
    learning rate ``lr``, in float64, each rounded once to float32:
    q_k = server_lr * p_k / sum_S p (the model fold), r_k = p_k / (K_k * lr) with
    K_k = E * ceil(n_k / B) (the variate fold), cs = 1 - sum_S p_k -- exactly 0 when S is every
    client -- and w_k = p_k / sum_S p (train_loss).  Returns (q, r, cs, w): float32 arrays and a float."""
    ns = np.asarray(ns, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    p = scaffold_weights(ns, weighting)[S]
    psum = float(np.sum(p))
    K = (int(epoch) * -(-ns[S] // int(batch_size))).astype(np.float64)
    q = (float(server_lr) * p / psum).astype(np.float32)
    r = (p / (K * float(lr))).astype(np.float32)
    cs = 0.0 if len(S) == len(ns) else float(np.float32(1.0 - psum))
    return q, r, cs, (p / psum).astype(np.float32)


SERVER_OPTS = ('avgm', 'adagrad', 'adam', 'yogi')
# the default server learning rates: 1 for momentum (FedAvgM's usual setting); 0.1 = 10^-1 for the
# adaptive rules, a point of the paper's grid {10^-3, 10^-2.5, ..., 10^1} -- a default, not a tuned value
SERVER_LR_DEFAULT = {'avgm': 1.0, 'adagrad': 0.1, 'adam': 0.1, 'yogi': 0.1}


def _check_server_opt(server_opt, server_lr, beta1, beta2, tau):
    """FedOpt's keyword checks (host only: before any device is touched)."""
    if server_opt not in SERVER_OPTS:
        raise ValueError("server_opt must be one of 'avgm', 'adagrad', 'adam', 'yogi'")
    if server_lr is not None and not float(server_lr) > 0.0:
        raise ValueError('server_lr must be > 0')
    if not float(tau) > 0.0:
        raise ValueError('tau must be > 0')
    for name, b in (('beta1', beta1), ('beta2', beta2)):
        if not 0.0 <= float(b) < 1.0:
            raise ValueError('%s must be in [0, 1)' % name)


def server_opt_scalars(server_opt, server_lr=None, beta1=0.9, beta2=0.99, tau=1e-3):
    """The host scalars of fs_aggregate_opt, computed in float64 and rounded once to float32:
    (rule, eta, beta1, omb1, beta2, omb2, tau) with omb = f32(1 - beta), the subtraction in float64
    on the caller's beta (not on its float32 rounding).  ``server_lr`` None: the rule's default
    (``SERVER_LR_DEFAULT``).  Returns the rule id (``_lib.OPT_*``) and six ``np.float32``."""
    _check_server_opt(server_opt, server_lr, beta1, beta2, tau)
    eta = SERVER_LR_DEFAULT[server_opt] if server_lr is None else float(server_lr)
    f = np.float32
    return (_lib.OPT_RULES[server_opt], f(eta), f(float(beta1)), f(1.0 - float(beta1)), f(float(beta2)),
            f(1.0 - float(beta2)), f(float(tau)))


def _check_qffl(q, weighting, lipschitz, clients='parallel'):
    """QFedAvg's keyword checks (host only: before any device is touched)."""
    if not float(q) >= 0.0 or float(q) == float('inf'):
        raise ValueError('q must be finite and >= 0')
    if weighting not in SCAFFOLD_WEIGHTINGS:
        raise ValueError("weighting must be 'size' or 'uniform'")
    if lipschitz is not None and not (0.0 < float(lipschitz) < float('inf')):
        raise ValueError('lipschitz must be finite and > 0')
    if clients != 'parallel':
        raise ValueError("QFedAvg needs clients='parallel': a chained client's W_j - W_g contains its predecessors' "
                         "work")


def qffl_lipschitz(lr, R, lipschitz=None):
    """q-FedAvg's Lipschitz estimate of every round (float64): ``lipschitz`` where given, else
    1 / lr_t with the round's decayed learning rate (``scaffold_lr_schedule``)."""
    if lipschitz is not None:
        return [float(lipschitz)] * int(R)
    return [1.0 / float(v) for v in scaffold_lr_schedule(lr, R)]


ROBUST_RULES = ('median', 'trimmed_mean', 'mean')
BYZANTINE_ATTACKS = ('sign_flip', 'gaussian', 'nan')


def _check_robust(rule, trim, clients='parallel'):
    """FedRobust's keyword checks (host only: before any device is touched)."""
    if rule not in ROBUST_RULES:
        raise ValueError("rule must be 'median', 'trimmed_mean' or 'mean'")
    if not (0.0 <= float(trim) < 0.5):
        raise ValueError('trim must be in [0, 0.5)')
    if clients != 'parallel':
        raise ValueError("FedRobust needs clients='parallel': a chained client's row holds its predecessors' work")


def robust_trim_count(rule, trim, M):
    """The trim count b of a round of M clients, as fs_plan_set_robust takes it: 'median' (M - 1) // 2,
    'trimmed_mean' floor(trim * M) in float64 clamped so that 2b < M, 'mean' 0."""
    M = int(M)
    if rule == 'median':
        return (M - 1) // 2
    if rule == 'mean':
        return 0
    return min(int(math.floor(float(trim) * float(M))), (M - 1) // 2)


def _check_robust_rounds(Ms, max_m):
    """ValueError for a round that no client trains in or whose client count exceeds ``max_m``."""
    for t, M in enumerate(Ms):
        if M < 1:
            raise ValueError('FedRobust: round %d samples no client' % t)
        if M > max_m:
            raise ValueError('FedRobust: round %d has M = %d clients, above fs_aggregate_robust_max_m() = %d'
                             % (t, M, max_m))


def _check_krum(f, m, clients='parallel'):
    """FedKrum's keyword checks (host only: before any device is touched)."""
    if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)):
        raise ValueError('f must be a fraction in [0, 0.5) or an int count >= 0')
    if isinstance(f, (int, np.integer)):
        if f < 0:
            raise ValueError('f must be a fraction in [0, 0.5) or an int count >= 0')
    elif not (0.0 <= float(f) < 0.5):
        raise ValueError('f must be a fraction in [0, 0.5) or an int count >= 0')
    if m is not None and (isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1):
        raise ValueError('m must be None (M - f) or an int count >= 1')
    if clients != 'parallel':
        raise ValueError("FedKrum needs clients='parallel': a chained client's row holds its predecessors' work")


def krum_counts(f, m, M):
    """(f, m) of a round of M clients: ``f`` an int count as it is, a fraction floor(f * M) in float64;
    ``m`` None: M - f.  ValueError unless M >= 2f + 3 (the paper's condition) and 1 <= m <= M - f."""
    M = int(M)
    fc = int(f) if isinstance(f, (int, np.integer)) else int(math.floor(float(f) * float(M)))
    if M < 2 * fc + 3:
        raise ValueError('FedKrum: a round of M = %d clients with f = %d needs M >= 2f + 3' % (M, fc))
    mc = M - fc if m is None else int(m)
    if not 1 <= mc <= M - fc:
        raise ValueError('FedKrum: m = %d is outside [1, M - f] = [1, %d]' % (mc, M - fc))
    return fc, mc


def _check_krum_rounds(Ms, f, m, max_m):
    """The (f, m) of every round; ValueError for a round above ``max_m`` clients or against krum_counts."""
    out = []
    for t, M in enumerate(Ms):
        if M > max_m:
            raise ValueError('FedKrum: round %d has M = %d clients, above fs_aggregate_krum_max_m() = %d'
                             % (t, M, max_m))
        out.append(krum_counts(f, m, M))
    return out


RFA_INITS = ('start', 'mean')
RFA_MAX_ITERS = 32


def _check_rfa(iters, nu, init, weighting, clients='parallel'):
    """FedRFA's keyword checks (host only: before any device is touched)."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= RFA_MAX_ITERS:
        raise ValueError('iters must be an int count in [0, %d]' % RFA_MAX_ITERS)
    if isinstance(nu, bool) or not isinstance(nu, (int, float, np.integer, np.floating)) \
            or not (float(nu) > 0.0 and math.isfinite(float(nu))):
        raise ValueError('nu must be a positive, finite number')
    if init not in RFA_INITS:
        raise ValueError("init must be 'start' or 'mean'")
    if weighting not in SCAFFOLD_WEIGHTINGS:
        raise ValueError("weighting must be 'size' or 'uniform'")
    if clients != 'parallel':
        raise ValueError("FedRFA needs clients='parallel': a chained client's row holds its predecessors' work")


def _check_rfa_rounds(Ms, max_m):
    """ValueError for a round with no client or above ``max_m`` clients."""
    for t, M in enumerate(Ms):
        if M < 1:
            raise ValueError('FedRFA: round %d has no client' % t)
        if M > max_m:
            raise ValueError('FedRFA: round %d has M = %d clients, above fs_aggregate_rfa_max_m() = %d'
                             % (t, M, max_m))


def _check_topk(ratio, error_feedback, clients='parallel'):
    """FedTopK's keyword checks (host only: before any device is touched)."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)):
        raise ValueError('ratio must be a fraction in (0, 1] or an int count >= 1')
    if isinstance(ratio, (int, np.integer)):
        if ratio < 1:
            raise ValueError('ratio as an int count must be >= 1')
    elif not (0.0 < float(ratio) <= 1.0):
        raise ValueError('ratio must be in (0, 1]')
    if not isinstance(error_feedback, (bool, np.bool_)):
        raise ValueError('error_feedback must be True or False')
    if clients != 'parallel':
        raise ValueError("FedTopK needs clients='parallel': a chained client's W_j - W_g holds its predecessors' work")


def topk_count(ratio, C, D):
    """The number of values a client uploads per round: ``ratio`` itself when it is an int count (at most
    C * D), else max(1, floor(ratio * C * D)) for a fraction in (0, 1]."""
    _check_topk(ratio, True)
    n = int(C) * int(D)
    if isinstance(ratio, (int, np.integer)):
        if ratio > n:
            raise ValueError('ratio as an int count must be at most C * D = %d' % n)
        return int(ratio)
    return max(1, int(math.floor(float(ratio) * n)))


def _check_dp(clip, noise_multiplier, noise_seed, weighting, adaptive, clients='parallel'):
    """DPFedAvg's keyword checks (host only: before any device is touched)."""
    def real(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
    if not real(clip) or not float(clip) > 0.0:
        raise ValueError('clip must be a number > 0 (inf: no clipping)')
    if not real(noise_multiplier) or not (0.0 <= float(noise_multiplier) < math.inf):
        raise ValueError('noise_multiplier must be finite and >= 0')
    if float(noise_multiplier) > 0.0 and math.isinf(float(clip)):
        raise ValueError('noise_multiplier > 0 needs a finite clip')
    if isinstance(noise_seed, bool) or not isinstance(noise_seed, (int, np.integer)) or not 0 <= noise_seed < 2 ** 64:
        raise ValueError('noise_seed must be an int in [0, 2^64)')
    if weighting not in SCAFFOLD_WEIGHTINGS:
        raise ValueError("weighting must be 'size' or 'uniform'")
    if adaptive is not None:
        if not isinstance(adaptive, dict) or set(adaptive) - {'quantile', 'lr', 'count_noise'} \
                or not {'quantile', 'lr'} <= set(adaptive):
            raise ValueError('adaptive must be None or dict(quantile=, lr=, count_noise=)')
        if not all(real(v) for v in adaptive.values()):
            raise ValueError('adaptive: quantile, lr and count_noise must be numbers')
        if not 0.0 <= float(adaptive['quantile']) <= 1.0:
            raise ValueError('adaptive: quantile must be in [0, 1]')
        if not 0.0 <= float(adaptive['lr']) < math.inf:
            raise ValueError('adaptive: lr must be finite and >= 0')
        if not 0.0 <= float(adaptive.get('count_noise', 0.0)) < math.inf:
            raise ValueError('adaptive: count_noise must be finite and >= 0')
        if math.isinf(float(clip)):
            raise ValueError('adaptive needs a finite clip')
    if clients != 'parallel':
        raise ValueError("DPFedAvg needs clients='parallel': a chained client's W_j - W_g holds its predecessors' work")


def byzantine_plan(N, byzantine):
    """``byzantine=`` checked and resolved (host only): None, or (sorted int64 ids, attack, scale, seed).
    ``ids``: the client ids given; ``fraction``: floor(fraction * N) ids fixed once from ``seed``
    (the first of a ``torch.randperm(N)`` of a private generator)."""
    if byzantine is None:
        return None
    bz = dict(byzantine)
    unknown = set(bz) - {'ids', 'fraction', 'attack', 'scale', 'seed'}
    if unknown:
        raise ValueError('unknown byzantine key(s) %s' % ', '.join(sorted(unknown)))
    if ('ids' in bz) == ('fraction' in bz):
        raise ValueError("byzantine needs exactly one of 'ids' and 'fraction'")
    attack, scale, seed = bz.get('attack', 'sign_flip'), float(bz.get('scale', 1.0)), int(bz.get('seed', 0))
    if attack not in BYZANTINE_ATTACKS:
        raise ValueError("byzantine attack must be 'sign_flip', 'gaussian' or 'nan'")
    if 'ids' in bz:
        ids = np.unique(np.asarray(list(bz['ids']), dtype=np.int64))
        if len(ids) and (ids[0] < 0 or ids[-1] >= N):
            raise ValueError('byzantine ids must be client ids in [0, %d)' % N)
    else:
        f = float(bz['fraction'])
        if not (0.0 <= f <= 1.0):
            raise ValueError('byzantine fraction must be in [0, 1]')
        g = torch.Generator()
        g.manual_seed(seed)
        ids = np.sort(torch.randperm(int(N), generator=g)[:int(math.floor(f * N))].numpy().astype(np.int64))
    return ids, attack, scale, seed


def byzantine_noise(seed, t, shape):
    """The N(0, 1) draws of ``attack='gaussian'`` for round ``t``: a private CPU generator seeded by
    (seed, t), float32 of ``shape`` (rows in ascending client id)."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(t)) % (1 << 62))
    return torch.randn(*shape, generator=g, dtype=torch.float32)


class Federation:
    """One algorithm call split into setup / rounds / results (bench.py drives the
    rounds one at a time through the same code path as the drop-ins)."""

    def __init__(self, algo, X_train, y_train, X_test, y_test, validloader, type, num_classes, D, lr, epoch,
                 batch_size, prox, mu, lambda_reg_if, lambda_reg, round, lr_p, clients, stats=None, verbose=True,
                 shuffle_device=True, options=None, participation=None, sample_seed=0, variant='reference',
                 server_lr=1.0, weighting='size', server_opt=None, qffl=None, robust=None, krum=None, rfa=None,
                 topk=None, dp=None):
        self.robust = algo == 'fedrobust'
        self.byz = None
        self.dp = algo == 'dpfedavg'
        if self.dp:
            # dp: dict(clip=, noise_multiplier=, noise_seed=, adaptive=, byzantine=) (tools.DPFedAvg); weighting
            # is the keyword above
            dpk = dict(dp or {})
            self.dp_clip0, self.dp_z = dpk.get('clip', 1.0), dpk.get('noise_multiplier', 1.0)
            self.dp_seed, self.dp_adaptive = dpk.get('noise_seed', 0), dpk.get('adaptive')
            _check_dp(self.dp_clip0, self.dp_z, self.dp_seed, weighting, self.dp_adaptive, clients)
            self.dp_uniform = weighting == 'uniform'
            self.byz = byzantine_plan(len(y_train), dpk.get('byzantine'))
        self.topk = algo == 'fedtopk'
        if self.topk:
            # topk: dict(ratio=, error_feedback=) (tools.FedTopK)
            tk = dict(topk or {})
            self.tk_ratio, self.tk_memory = tk.get('ratio', 0.01), tk.get('error_feedback', True)
            _check_topk(self.tk_ratio, self.tk_memory, clients)
            self.tk_count = topk_count(self.tk_ratio, num_classes, D)
        self.rfa = algo == 'fedrfa'
        if self.rfa:
            # rfa: dict(iters=, nu=, init=, byzantine=) (tools.FedRFA); weighting is the keyword above
            rf = dict(rfa or {})
            self.rf_T, self.rf_nu, self.rf_init = rf.get('iters', 3), rf.get('nu', 1e-6), rf.get('init', 'start')
            _check_rfa(self.rf_T, self.rf_nu, self.rf_init, weighting, clients)
            self.rf_uniform = weighting == 'uniform'
            self.byz = byzantine_plan(len(y_train), rf.get('byzantine'))
        self.krum = algo == 'fedkrum'
        if self.krum:
            # krum: dict(f=, m=, byzantine=) (tools.FedKrum)
            kr = dict(krum or {})
            self.kr_f, self.kr_m = kr.get('f', 0.1), kr.get('m')
            _check_krum(self.kr_f, self.kr_m, clients)
            self.byz = byzantine_plan(len(y_train), kr.get('byzantine'))
        if self.robust:
            # robust: dict(rule=, trim=, byzantine=) (tools.FedRobust)
            rb = dict(robust or {})
            self.rb_rule, self.rb_trim = rb.get('rule', 'median'), float(rb.get('trim', 0.1))
            _check_robust(self.rb_rule, self.rb_trim, clients)
            self.byz = byzantine_plan(len(y_train), rb.get('byzantine'))
        self.qffl = algo == 'qfedavg'
        if self.qffl:
            # qffl: dict(q=, lipschitz=) (tools.QFedAvg); weighting is the keyword above
            qf = dict(qffl or {})
            self.qf_q, self.qf_lipschitz = float(qf.get('q', 1.0)), qf.get('lipschitz')
            _check_qffl(self.qf_q, weighting, self.qf_lipschitz, clients)
        self.fedopt = algo == 'fedopt'
        if self.fedopt:
            # server_opt: dict(rule=, server_lr=, beta1=, beta2=, tau=, v0=) (tools.FedOpt)
            so = dict(server_opt or {})
            self.opt_v0 = so.pop('v0', None)
            so.setdefault('rule', 'adam')
            self.opt_tau = float(so.get('tau', 1e-3))      # the caller's tau: v0 = tau^2 in float64, rounded once
            self.opt_scalars = server_opt_scalars(so.pop('rule'), **so)
            if self.opt_v0 is not None and not float(self.opt_v0) >= 0.0:
                raise ValueError('v0 must be >= 0')
            if clients != 'parallel':
                raise ValueError("FedOpt needs clients='parallel': a chained client's W_j - W_g contains its "
                                 "predecessors' work")
        if algo == 'fednova':
            _check_nova(variant, clients)
        self.scaffold = algo == 'scaffold'
        if self.scaffold:
            if clients != 'parallel':
                raise ValueError("Scaffold needs clients='parallel': every client starts from the round's global model")
            _check_scaffold(type, prox, batch_size, weighting, server_lr)
        opts = dict(OPTIONS)
        for k, v in (options or {}).items():
            if k not in opts:
                raise ValueError('unknown Federation option %r (known: %s)' % (k, ', '.join(sorted(OPTIONS))))
            opts[k] = v
        if opts['fedamw_shuffle'] not in ('early', 'late'):
            raise ValueError("fedamw_shuffle must be 'early' or 'late'")
        self.options = opts
        client_eval = _client_eval_request(stats, validloader is not None)
        local_eval = _local_eval_request(stats)
        # (training labels: only this rank's clients, below -- in sharded mode the other ranks'
        # entries of X_train / y_train need only have the right lengths)
        _check_inputs(type, X_train, y_train, num_classes, batch_size, epoch, round, y_test,
                      validloader.dataset.tensors[1] if validloader is not None else None, train_labels=False)
        if clients not in ('sequential', 'parallel'):
            raise ValueError("clients must be 'sequential' or 'parallel'")
        self.chained = clients == 'sequential'
        self.rank, nranks = dist.world()
        # partial participation: self.sched[t] = the sorted ids of the clients that train in round t
        # (None: every client, every round -- the code path without the keyword, untouched)
        self.sched = None
        if participation is not None:
            if algo not in ('fedavg', 'fedprox', 'fednova', 'scaffold', 'fedopt', 'qfedavg', 'fedrobust', 'fedkrum',
                            'fedrfa', 'fedtopk', 'dpfedavg'):
                raise NotImplementedError('participation is implemented for FedAvg, FedProx, FedNova, Scaffold, '
                                          'FedOpt, QFedAvg and FedRobust only')
            if self.chained:
                raise ValueError("participation needs clients='parallel': every sampled client starts from the "
                                 "round's global model (clients='sequential' chains all clients)")
            if nranks > 1:
                raise NotImplementedError('participation over more than one torch.distributed rank is not implemented')
            self.sched = _participation.make_schedule(len(y_train), int(round), participation, sample_seed)
        if algo == 'fednova' and nranks > 1:
            raise NotImplementedError('FedNova over more than one torch.distributed rank is not implemented')
        if self.scaffold and nranks > 1:
            raise NotImplementedError('Scaffold over more than one torch.distributed rank is not implemented')
        if self.fedopt and nranks > 1:
            # (delta would need its all-reduce before the nonlinear step)
            raise NotImplementedError('FedOpt over more than one torch.distributed rank is not implemented')
        if self.qffl and nranks > 1:
            # (S, the norms and H would need their all-reduce before the step)
            raise NotImplementedError('QFedAvg over more than one torch.distributed rank is not implemented')
        if self.robust:
            if nranks > 1:
                # (an order statistic over all clients' rows is no sum of the ranks' parts)
                raise NotImplementedError('FedRobust over more than one torch.distributed rank is not implemented')
            self.rb_M = [len(y_train)] * int(round) if self.sched is None else [len(S) for S in self.sched]
            _check_robust_rounds(self.rb_M, engine.robust_max_m())
            self.rb_b = [robust_trim_count(self.rb_rule, self.rb_trim, M) for M in self.rb_M]
        if self.krum:
            if nranks > 1:
                # (the distances need all clients' rows)
                raise NotImplementedError('FedKrum over more than one torch.distributed rank is not implemented')
            self.kr_M = [len(y_train)] * int(round) if self.sched is None else [len(S) for S in self.sched]
            self.kr_fm = _check_krum_rounds(self.kr_M, self.kr_f, self.kr_m, engine.krum_max_m())
        if self.rfa:
            if nranks > 1:
                # (the distances need all clients' rows)
                raise NotImplementedError('FedRFA over more than one torch.distributed rank is not implemented')
            self.rf_M = [len(y_train)] * int(round) if self.sched is None else [len(S) for S in self.sched]
            _check_rfa_rounds(self.rf_M, engine.rfa_max_m())
        if self.topk and nranks > 1:
            # (a client's residual lives with its row; the thresholded fold has no all-reduce form here)
            raise NotImplementedError('FedTopK over more than one torch.distributed rank is not implemented')
        if self.dp and nranks > 1:
            # (every update's norm needs its whole row, and the noise is added once)
            raise NotImplementedError('DPFedAvg over more than one torch.distributed rank is not implemented')
        self.sharded = (not self.chained) and nranks > 1
        if self.sharded and len(y_train) < nranks:
            raise ValueError("clients='parallel' over %d ranks needs at least one client per rank (got %d clients)"
                             % (nranks, len(y_train)))
        self.algo, self.stats, self.verbose = algo, stats, verbose
        self.C, self.E, self.B, self.R, self.D = int(num_classes), int(epoch), int(batch_size), int(round), int(D)
        self.lr, self.lr_p, self.prox, self.mu, self.reg, self.lam = lr, lr_p, prox, mu, lambda_reg_if, lambda_reg
        C, E, B, R = self.C, self.E, self.B, self.R
        N = len(y_train)
        self.N = N
        ns = np.array([len(y) for y in y_train], dtype=np.int64)
        self.ns = ns
        self.shards = dist.shard_lpt(dist.client_work(ns, E, B), nranks) if self.sharded else [np.arange(N)]
        self.mine = self.shards[self.rank] if self.sharded else self.shards[0]
        mine = self.mine
        loss = self.loss = _loss_of(type)
        if loss == 'ce':
            _check_labels([y_train[j] for j in mine], num_classes, 'training')
        dev = _device()

        # model init + mixture weights exactly as the reference (tools.py:330-333, 414-417)
        W_init = init_weights(D, C)
        self.p_all = torch.tensor(ns / sum(ns), dtype=torch.float32)

        self.feats = engine.Features([torch.as_tensor(X_train[j]) for j in mine],
                                     [torch.as_tensor(y_train[j]) for j in mine], D, dev,
                                     float_targets=loss == 'mse')
        ld = self.ld = self.feats.ld
        # sharded FedAMW: the p-solve's client axis is rank-major blocks of L columns (dist.py)
        self.zshard = algo == 'fedamw' and self.sharded
        if self.zshard:
            self.L, self.pos = dist.solver_layout(self.shards)
            self.pos_dev = torch.from_numpy(self.pos).to(dev)
        self.trainer = engine.LocalTrainer(self.feats, C, B, E, chained=self.chained,
                                           rows=self.L if self.zshard else None, prox=prox, loss=loss)
        self.evaluator = engine.Evaluator(X_test, y_test, D, C, dev, ld, loss=loss)
        self.W_g = torch.zeros(C, ld, device=dev, dtype=torch.float32)
        self.W_g[:, :D].copy_(W_init)
        p_dev = self.p_all.to(dev)
        self.p_mine = p_dev[torch.from_numpy(mine).to(dev)] if self.sharded else p_dev
        self.mixture = None
        self.inv = (torch.from_numpy(np.argsort(np.concatenate(self.shards), kind='stable')).to(dev)
                    if self.sharded else None)
        if algo == 'fedamw':
            Xv, yv = validloader.dataset.tensors[:2]
            Bv = int(validloader.batch_size)
            if not isinstance(validloader.sampler, torch.utils.data.RandomSampler):
                raise NotImplementedError('validloader must shuffle (exp.py:99)')
            if self.zshard:
                Ns = nranks * self.L
                p0 = torch.zeros(Ns, dtype=torch.float32)
                p0[torch.from_numpy(self.pos)] = self.p_all
                self.mixture = engine.Mixture(Xv, yv, D, C, Ns, Bv, p0, dev, ld, loss=loss)
                # the qmc solver reads the all-gathered rank blocks as they land (no layout copy);
                # which layout to gather is decided again every round, right before the
                # all-gather (round()), under the tuning the enqueueing thread has then
                self.nranks = nranks
                self.Z_local = torch.empty(self.mixture.nv, C * self.L, device=dev, dtype=torch.float32)
                lo = self.rank * self.L
                self.p_slice = lambda p: p[lo:lo + len(mine)]
                self.agg = engine.Aggregator(len(mine), C, ld, dev)
            else:
                self.mixture = engine.Mixture(Xv, yv, D, C, N, Bv, self.p_all, dev, ld, loss=loss)
                self.agg = engine.Aggregator(N, C, ld, dev)
            self.p_hist = torch.empty(R, N, dtype=torch.float32, device=dev)
        else:
            self.agg = engine.Aggregator(len(mine), C, ld, dev)
        self.loss_hist = torch.empty(R, len(mine), dtype=torch.float64, device=dev)
        # FedNova (tools.py:383-410): FedAvg's round with fs_aggregate_nova as its aggregate.
        # 'reference': the reference's host scalars, mode 1 with q = p; 'updates': mode 2 with
        # q = a.  train_loss keeps the plain p (tools.py:400).  Under participation the scalars are
        # taken over each round's sample (below) and set before that round's aggregate.
        self.nova = None
        p_plan = self.p_mine
        if algo == 'fednova':
            if variant == 'reference':
                _, b, te, s0 = nova_reference_coefficients(ns, E, B)
                self.nova = (_lib.NOVA_REFERENCE, b.to(dev), te, s0)
            else:
                p_plan = nova_update_coefficients(ns, E, B)[1].to(dev)
                self.nova = (_lib.NOVA_UPDATES, None, 1.0, 1.0)
        if self.sched is not None:
            # the whole schedule goes to the device once, before round 0: per round the sampled ids
            # ascending (the aggregate's fold order) and in dispatch order (LPT over the sample:
            # steps descending, stable), and q = n[S] / sum(n[S]) as tools.py:333 restricted to S.
            # [R][max M], a round reads its first M_t entries; held for the whole run (the
            # launches read them asynchronously).  Unsampled clients' losses stay NaN.
            self.loss_hist.fill_(float('nan'))
            Mx = max([len(S) for S in self.sched] + [1])
            sel_h, ord_h = np.zeros((R, Mx), np.int32), np.zeros((R, Mx), np.int32)
            q_h = torch.zeros(R, Mx, dtype=torch.float32)
            self.q_host = []
            for t, S in enumerate(self.sched):
                q = torch.tensor(ns[S] / sum(ns[S]), dtype=torch.float32)
                self.q_host.append(q)
                sel_h[t, :len(S)], ord_h[t, :len(S)], q_h[t, :len(S)] = S, self.trainer.sel_order(S), q
            if self.nova is not None:
                # per-round b / te / s0 (reference) or a in q's place (updates), uploaded once here
                b_h = torch.ones(R, Mx, dtype=torch.float32)
                self.nova_round = []
                for t, S in enumerate(self.sched):
                    if len(S) == 0:
                        self.nova_round.append((1.0, 1.0))
                    elif self.nova[0] == _lib.NOVA_REFERENCE:
                        _, b, te, s0 = nova_reference_coefficients(ns[S], E, B)
                        b_h[t, :len(S)] = b
                        self.nova_round.append((te, s0))
                    else:
                        q_h[t, :len(S)] = nova_update_coefficients(ns[S], E, B)[1]
                        self.nova_round.append((1.0, 1.0))
                self.nova_b_dev = b_h.to(dev)
            if self.scaffold:
                q_h.zero_()          # SCAFFOLD's own q (below), not n[S] / sum(n[S])
            self.sel_dev = torch.from_numpy(sel_h).to(dev)
            self.sel_order_dev = torch.from_numpy(ord_h).to(dev)
        if self.scaffold:
            # SCAFFOLD: the variates (all zero before round 0) and the q / r / cs tables of every
            # round, built on the host once and uploaded before round 0 (r and cs change with the
            # round's lr and sample; the launches read them asynchronously)
            self.c_var = torch.zeros(C, ld, device=dev, dtype=torch.float32)
            self.ci_var = torch.zeros(N, C, ld, device=dev, dtype=torch.float32)
            lrs = scaffold_lr_schedule(lr, R)
            Mx = N if self.sched is None else q_h.shape[1]
            if self.sched is None:
                q_h = torch.zeros(R, Mx, dtype=torch.float32)
            r_h = torch.zeros(R, Mx, dtype=torch.float32)
            self.sc_cs, self.sc_w = [], []
            for t in range(R):
                S = np.arange(N) if self.sched is None else self.sched[t]
                q, r, cs, w = scaffold_round_coefficients(ns, S, E, B, lrs[t], server_lr, weighting)
                q_h[t, :len(S)], r_h[t, :len(S)] = torch.from_numpy(q), torch.from_numpy(r)
                self.sc_cs.append(cs)
                self.sc_w.append(torch.from_numpy(w))
            self.sc_r_dev = r_h.to(dev)
            self.sc_q_dev = q_h.to(dev)
            self.c_hist = torch.empty(R, C, ld, device=dev) if (stats is not None and stats.get('trace')) else None
        if self.sched is not None:
            self.q_dev = q_h.to(dev)
        self.eval_hist = torch.empty(R, 2, dtype=torch.float64, device=dev)
        self.W_hist = torch.empty(R, C, ld, device=dev) if (stats is not None and stats.get('trace')) else None
        # stats['client_eval']: every local model of the round scored on the test and / or the
        # validation rows (engine.ClientEvaluator) into a device history [R][len(mine)][2]
        self.client_eval = {}
        for which in client_eval:
            zs = which == 'val' and self.zshard       # this rank's Z block: L columns, padding clients last
            ce = engine.ClientEvaluator(self.evaluator.f if which == 'test' else self.mixture.f, C,
                                        self.L if zs else len(mine), loss=loss)
            self.client_eval[which] = (ce, torch.zeros(R, len(mine), 2, dtype=torch.float64, device=dev),
                                       torch.empty(self.L, 2, dtype=torch.float64, device=dev) if zs else None)
        # stats['local_eval']: the round's global model and / or every client's own model scored
        # on this rank's clients' own rows (engine.LocalEvaluator) into device histories [R][len(mine)][2]
        self.local_eval = engine.LocalEvaluator(self.feats, C, loss=loss) if local_eval else None
        self.local_hist = {which: torch.zeros(R, len(mine), 2, dtype=torch.float64, device=dev)
                           for which in local_eval}
        self.n_val_pass = R if algo == 'fedamw' else 0
        self.side = torch.cuda.Stream(device=dev)    # FedAMW validation shuffles of round t+1 run here
        # the native round driver (csrc/round.hip): one call per round phase, training shuffles
        # replayed into a double-buffered slot on its side stream
        self.plan = engine.RoundPlan(self.trainer, self.W_g, self.loss_hist, p=p_plan,
                                     aggregator=self.agg if self.mixture is None else None,
                                     evaluator=self.evaluator, eval_hist=self.eval_hist, prox=prox, mu=mu,
                                     reg=lambda_reg_if, lam=lambda_reg, chained=self.chained,
                                     shuffle_device=shuffle_device, shuffle_after_train=self.mixture is not None)
        # FedAMW: round t+1's shuffles (training and validation passes) are generated behind
        # round t's local training, beside its p-solve (one to 32 CUs busy), not beside the
        # training kernel, whose groups would wait for the CUs they hold
        # FedAvg / FedProx with device-replayed shuffles: generate them K rounds per launch
        # (options['shuffle_chunk'], default 8; 1 = per round), one chunk ahead of the rounds that
        # use them, so consecutive rounds run with no cross-stream wait between them.  FedAMW
        # keeps per-round shuffles (its validation shuffles are double-buffered per round).
        if self.nova is not None and self.sched is None:
            self.plan.set_nova(*self.nova)
        if self.fedopt:
            # FedOpt: FedAvg's round with fs_aggregate_opt as its aggregate.  m0 = 0, v0 = tau^2 (the
            # paper's initialisation) unless given; the scalars do not change with the round
            tau = self.opt_tau
            self.opt_m = torch.zeros(C, ld, device=dev, dtype=torch.float32)
            self.opt_v = torch.full((C, ld), tau * tau if self.opt_v0 is None else float(self.opt_v0), device=dev,
                                    dtype=torch.float32)
            self.plan.set_server_opt(self.opt_scalars[0], self.opt_m, self.opt_v, *self.opt_scalars[1:])
            trace = stats is not None and stats.get('trace')
            self.m_hist = torch.empty(R, C, ld, device=dev) if trace else None
            self.v_hist = torch.empty(R, C, ld, device=dev) if trace else None
        if self.qffl:
            # q-FedAvg: FedAvg's round with fs_aggregate_qffl as its aggregate, after one local
            # evaluation of the round's starting model and fs_qffl_coef.  p_k over ALL N clients
            # (H normalises), per round the sampled ones' in ascending id; L_t on the host
            p64 = scaffold_weights(ns, weighting)
            Mx = N if self.sched is None else self.sel_dev.shape[1]
            p_h = np.zeros((R, Mx), np.float32)
            for t in range(R):
                S = np.arange(N) if self.sched is None else self.sched[t]
                p_h[t, :len(S)] = p64[S].astype(np.float32)
            self.qf_p_dev = torch.from_numpy(p_h).to(dev)
            self.qf_L = qffl_lipschitz(lr, R, self.qf_lipschitz)
            self.qf_eval = self.local_eval or engine.LocalEvaluator(self.feats, C, loss=loss)
            self.qf_F = torch.zeros(R, N, 2, dtype=torch.float64, device=dev)
            self.qf_u = torch.zeros(Mx, dtype=torch.float32, device=dev)
            self.qf_g = torch.zeros(Mx, dtype=torch.float32, device=dev)
            self.qf_S = torch.zeros(C, ld, dtype=torch.float32, device=dev)
            self.qf_n = torch.full((R, Mx), float('nan'), dtype=torch.float64, device=dev)
            self.qf_hc = torch.zeros(R, 2, dtype=torch.float64, device=dev)
            self.qf_nws = self.agg.qffl_ws()
        if self.robust:
            # FedAvg's round with fs_aggregate_robust as its aggregate; b follows each round's own
            # client count inside the plan ('mean': trim 0)
            self.plan.set_robust(True, 'median' if self.rb_rule == 'median' else 'trimmed_mean',
                                 self.rb_trim if self.rb_rule == 'trimmed_mean' else 0.0)
        if self.krum:
            # FedAvg's round with fs_aggregate_krum as its aggregate; every round's ids and scores land in
            # that round's row of the two histories (the setter is called again before each round)
            self.kr_pick = torch.full((R, self.N), -1, dtype=torch.int32, device=dev)
            self.kr_score = torch.full((R, self.N), float('nan'), dtype=torch.float64, device=dev)
            self.kr_ws = self.agg.krum_ws()
        if self.rfa:
            # FedAvg's round with fs_aggregate_rfa as its aggregate; every round's weights, distances and
            # objectives land in that round's row of the histories (the setter is called again before each round)
            self.rf_b = torch.full((R, self.N), float('nan'), dtype=torch.float32, device=dev)
            self.rf_dist = torch.full((R, self.N), float('nan'), dtype=torch.float64, device=dev)
            self.rf_obj = torch.full((R, int(self.rf_T) + 2), float('nan'), dtype=torch.float64, device=dev)
            self.rf_ws = self.agg.rfa_ws()
        if self.topk:
            # FedAvg's round with fs_aggregate_topk as its aggregate; the residuals (all zero before round 0)
            # stay with their clients, every round's thresholds and kept counts land in that round's row
            # of the histories (the setter is called again before each round)
            self.tk_e = torch.zeros(N, C, ld, device=dev, dtype=torch.float32) if self.tk_memory else None
            self.tk_tau = torch.full((R, self.N), float('nan'), dtype=torch.float32, device=dev)
            self.tk_kept = torch.full((R, self.N), -1, dtype=torch.int32, device=dev)
            self.tk_ws = self.agg.topk_ws()
            self.tk_rnorm = torch.zeros(R, dtype=torch.float64, device=dev) if stats is not None else None
        if self.dp:
            # FedAvg's round with fs_aggregate_dp as its aggregate; every round's coefficients, norms and state
            # land in that round's row of the histories (the setter is called again before each round), the
            # adaptive clip lives on the device
            self.dp_c = torch.zeros(R, self.N, dtype=torch.float32, device=dev)
            self.dp_r = torch.full((R, self.N), float('nan'), dtype=torch.float64, device=dev)
            self.dp_state = torch.full((R, engine.DP_STATE), float('nan'), dtype=torch.float64, device=dev)
            self.dp_clip_dev = (torch.full((1,), float(self.dp_clip0), dtype=torch.float64, device=dev)
                                if self.dp_adaptive is not None else None)
            self.dp_ws = self.agg.dp_ws()
        self.chunk = 1
        if self.mixture is None and shuffle_device and self.sched is None:   # (subset rounds: per-round slots)
            self.chunk = max(1, min(int(opts['shuffle_chunk']), R))
            if self.chunk > 1:
                self.plan.set_chunk(self.chunk)
        # round t's test-set evaluation is deferred into round t+1's training launch when that
        # launch leaves CUs idle (options['defer_eval'] = False: an evaluation launch per round)
        self.defer_eval = bool(opts['defer_eval'])
        self._prepared = 0              # next round whose shuffles are to be prepared
        self._train_done = None
        self.t = 0
        self.events = None              # a list: round() appends (phase, start, end) HIP timing events

    def _prepare(self, t):
        """Draw round t's shuffle seeds (torch's global CPU generator, in the reference's
        order: train passes client-major, then validation passes, then the test pass), replay
        the training shuffles into the plan's slot t % 2 (on its side stream) and enqueue the validation shuffles (FedAMW) on the side stream."""
        N, E = self.N, self.E
        if self.sched is not None:
            # only the sampled clients' passes draw (ascending client id, epoch-minor), then the
            # test pass: M_t * E + n_val_pass + 1 passes
            S = self.sched[t]
            seeds = rng.draw_pass_seeds(len(S) * E + self.n_val_pass + 1)
            self.plan.shuffle_subset(seeds[:len(S) * E], S, t)
            return
        seeds = rng.draw_pass_seeds(N * E + self.n_val_pass + 1)
        self.plan.shuffle(seeds[:N * E].reshape(N, E)[self.mine].reshape(-1), t)
        if self.mixture is not None:
            if self._train_done is not None:
                self.side.wait_event(self._train_done)
            self.mixture.prepare(seeds[N * E:N * E + self.n_val_pass], t % 2, self.side)

    def _prepare_upto(self, end):
        """Prepare the shuffles of every round before ``min(end, R)`` not prepared yet, in order."""
        while self._prepared < min(end, self.R):
            self._prepare(self._prepared)
            self._prepared += 1
            if self._prepared == self.R and self.chunk > 1:
                self.plan.flush()

    def round(self):
        """Run round t (tools.py:337-352 / 364-379 / 427-462) -- all launches async.  Round
        t+1's seeds are drawn (and its shuffles replayed) after round t is
        enqueued, so the host work overlaps the GPU; the draw pattern is data-independent,
        so this leaves the generator exactly where the reference leaves it after each call."""
        t = self.t
        if t == 0:
            self._prepare_upto(2 * self.chunk if self.chunk > 1 else 1)
        self.lr = update_learning_rate(t, self.lr, self.R)
        P = _lib.PHASE_TRAIN, _lib.PHASE_AGGREGATE, _lib.PHASE_EVAL
        if t + 1 < self.R and self.defer_eval:
            # this round's evaluation rides on round t+1's training launch where that launch
            # leaves CUs idle (fs_plan_round, FS_PHASE_EVAL_DEFER); same arithmetic per row
            P = P[0], P[1], P[2] | _lib.PHASE_EVAL_DEFER
        ev = self.events

        def timed(name, fn):
            if ev is None:
                return fn()
            a, b = _lib.Timer(), _lib.Timer()     # no system-scope release (fs_timer_*)
            a.record()
            out = fn()
            b.record()
            ev.append((name, a, b))
            return out

        if self.scaffold:
            self.plan.set_scaffold(True, self.c_var, self.ci_var, self.sc_r_dev[t], self.sc_cs[t])
        if self.qffl:
            # F_k(W_g) on every client's own rows (all N, also under participation: fs_eval_clients
            # has no subset form), then u and g of the sampled ones, all on the device
            M_t = self.N if self.sched is None else len(self.sched[t])
            timed('qffl_eval', lambda: self.qf_eval.run(self.W_g, 0, self.qf_F[t]))
            timed('qffl_coef', lambda: engine.qffl_coef(self.qf_F[t], self.qf_p_dev[t][:M_t], self.qf_q, self.qf_L[t],
                                                        self.qf_u, self.qf_g,
                                                        None if self.sched is None else self.sel_dev[t][:M_t]))
            self.plan.set_qffl(True, self.qf_g, self.qf_L[t], self.qf_S, self.qf_n[t], self.qf_hc[t], self.qf_nws)
        if self.krum:
            # (f + 1/2) / M: the fraction whose floor(. * M) is this round's f inside the plan
            f_t, m_t = self.kr_fm[t]
            self.plan.set_krum(True, (f_t + 0.5) / self.kr_M[t], m_t, self.kr_pick[t], self.kr_score[t], self.kr_ws)
        if self.rfa:
            self.plan.set_rfa(True, self.rf_T, self.rf_nu, self.rf_init, self.rf_uniform, self.rf_dist[t],
                              self.rf_b[t], self.rf_obj[t], self.rf_ws)
        if self.topk:
            self.plan.set_topk(True, self.tk_count, self.tk_e, self.tk_tau[t], self.tk_kept[t], self.tk_ws)
        if self.dp:
            self.plan.set_dp(True, self.dp_clip0, self.dp_z, self.dp_seed, self.dp_uniform, self.dp_adaptive,
                             self.dp_clip_dev, self.dp_c[t], self.dp_r[t], self.dp_state[t], self.dp_ws, cols=self.D)
        if self.sched is not None:
            M = len(self.sched[t])

            if self.nova is not None:
                self.plan.set_nova(self.nova[0], self.nova_b_dev[t] if self.nova[1] is not None else None,
                                   *self.nova_round[t])

            def plan_round(phases):
                self.plan.round_subset(t, self.lr, phases, self.sel_dev[t], self.sel_order_dev[t],
                                       self.qf_u if self.qffl else self.q_dev[t], M)
        else:
            def plan_round(phases):
                self.plan.round(t, self.lr, phases,
                                self.sc_q_dev[t] if self.scaffold else self.qf_u if self.qffl else None)
        timed('train', lambda: plan_round(P[0]))
        if self.byz is not None:
            timed('byzantine', lambda: self._corrupt(t))
        # (under participation the two evaluations of the clients' OWN models below still score all
        # N rows of W_out -- stale rows of clients that sat the round out, zeros before a client's
        # first round -- and results() masks the unsampled ones to NaN: both evaluators walk the
        # clients x params buffer by position.  At 10 % participation that is 10 x the work this
        # stats path needs; scoring the sampled rows only would take an index table in
        # fs_mix_z / fs_eval_clients, not done here.)
        if 'test' in self.client_eval:
            ce, hist, _ = self.client_eval['test']
            timed('client_eval_test', lambda: ce.run(self.trainer.W_out, len(self.mine), hist[t]))
        if 'own' in self.local_hist:
            timed('local_eval_own', lambda: self.local_eval.run(self.trainer.W_out, self.C * self.ld,
                                                                self.local_hist['own'][t]))
        cev = self.client_eval.get('val')
        early = False
        if self.mixture is not None:
            self._train_done = torch.cuda.Event()
            self._train_done.record()
            # FedAMW: round t+1's shuffles are enqueued now (nothing else draws from the global
            # generator in between, so the draw order is unchanged) and the p-solve waits for the
            # validation shuffles: they run beside the Z GEMM, not on the CUs of the p-solve's
            # workgroups (options['fedamw_shuffle'] = 'late': after the round, beside the p-solve)
            early = self.t + 1 < self.R and self.options['fedamw_shuffle'] != 'late'
            if early:
                self._prepare_upto(t + 2)
        if self.zshard:
            # tools.py:435-453 sharded: this rank's Z columns, one all-gather, the replicated
            # p-solve, then this rank's partial aggregate with its learned p and one all-reduce
            self.p_hist[t].copy_(self.mixture.p[self.pos_dev])
            # the blocked layout only where fs_mix_solve_blocked covers the shape under THIS
            # thread's tuning now (a tuning change between rounds, or a round
            # enqueued from another thread, must not leave a blocked Z for a solver that
            # cannot read it)
            self.mixture.blocks = (self.nranks if self.nranks > 1 and self.mixture.blocked_covers(self.R) else 1)
            timed('z', lambda: self.mixture.z_block(self.trainer.W_out, self.L, self.Z_local))
            if cev is not None:       # Z_local is the standard layout at N = L; never the rank-blocked Z
                timed('client_eval_val', lambda: cev[0].run_z(self.Z_local, self.L, cev[2]))
                cev[1][t].copy_(cev[2][:len(self.mine)])
            timed('z_allgather', lambda: dist.allgather_z(self.Z_local, self.C, self.mixture.Z,
                                                          blocked=self.mixture.blocks > 1))
            if early:
                torch.cuda.current_stream().wait_stream(self.side)
            p = timed('solve', lambda: self.mixture.solve(None, None, self.lr_p, slot=t % 2, z=False))
            self.agg.run(self.trainer.W_out, self.p_slice(p), self.W_g)
            dist.allreduce_sum_(self.W_g)
            self.plan.round(t, self.lr, P[2])
        elif self.mixture is not None:
            self.p_hist[t].copy_(self.mixture.p)
            timed('z', lambda: self.mixture.z_block(self.trainer.W_out, self.N, self.mixture.Z))
            if cev is not None:       # the p-solve's Z: no second GEMM
                timed('client_eval_val', lambda: cev[0].run_z(self.mixture.Z, self.N, cev[1][t]))
            if early:
                torch.cuda.current_stream().wait_stream(self.side)
            p = timed('solve', lambda: self.mixture.solve(None, None, self.lr_p, slot=t % 2, z=False))
            self.agg.run(self.trainer.W_out, p, self.W_g)
            self.plan.round(t, self.lr, P[2])
        elif self.sharded:
            self.plan.round(t, self.lr, P[1])
            dist.allreduce_sum_(self.W_g)
            self.plan.round(t, self.lr, P[2])
        else:
            plan_round(P[1] | P[2])
        if 'global' in self.local_hist:     # the W_g that test_loss[t] scores (read only: a deferred test
            # evaluation, which reads it in round t+1's training launch, is not disturbed)
            timed('local_eval_global', lambda: self.local_eval.run(self.W_g, 0, self.local_hist['global'][t]))
        if self.W_hist is not None:
            self.W_hist[t].copy_(self.W_g)
        if self.scaffold and self.c_hist is not None:
            self.c_hist[t].copy_(self.c_var)
        if self.fedopt and self.m_hist is not None:
            self.m_hist[t].copy_(self.opt_m)
            self.v_hist[t].copy_(self.opt_v)
        if self.topk and self.tk_rnorm is not None and self.tk_e is not None:
            self.tk_rnorm[t] = torch.linalg.vector_norm(self.tk_e, dtype=torch.float64)
        self.t += 1
        if self.chunk > 1:
            if t % self.chunk == 0 and t >= self.chunk:      # chunk c started: prepare chunk c + 1
                self._prepare_upto(t + 2 * self.chunk)
        elif self.t < self.R and not early:
            self._prepare_upto(self.t + 1)

    def _corrupt(self, t):
        """``byzantine=``: overwrite the corrupted clients' rows of ``W_out`` that round t sampled, after
        TRAIN and before AGGREGATE, on the current stream (a few torch ops on at most f * M rows)."""
        ids, attack, scale, seed = self.byz
        rows = ids if self.sched is None else np.intersect1d(ids, self.sched[t])
        if len(rows) == 0:
            return
        idx = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.W_g.device)
        W = self.trainer.W_out
        if attack == 'sign_flip':
            W[idx] = self.W_g - scale * (W[idx] - self.W_g)
        elif attack == 'gaussian':
            z = byzantine_noise(seed, t, (len(rows), self.C, self.D)).to(self.W_g.device)
            W[idx, :, :self.D] = self.W_g[:, :self.D] + scale * z
        else:
            W[idx, :, :self.D] = float('nan')

    def _mask_unsampled(self, hist):
        """hist [R, N, 2] of every client's OWN model per round: under partial participation a
        copy with NaN for the clients that did not train in a round (their W_out rows are stale)."""
        if self.sched is None:
            return hist
        keep = torch.zeros(hist.shape[0], hist.shape[1], dtype=torch.bool)
        for t, S in enumerate(self.sched):
            keep[t, torch.from_numpy(S)] = True
        hist = hist.clone()
        hist[~keep.to(hist.device)] = float('nan')
        return hist

    def results(self):
        """Single host sync: (train_loss, test_loss, test_acc) CPU float32 tensors."""
        R, D = self.t, self.D
        if 0 < R and self.defer_eval:
            self.plan.eval_flush()                       # completes a deferred evaluation, if any (ABI 15)
        self.trainer.check_errors()
        if self.mixture is not None:
            self.mixture.check_errors()
        loss_hist = self.loss_hist[:R]
        if self.sharded:
            loss_hist = dist.allgather_rows(loss_hist.t().contiguous(), [len(s) for s in self.shards]).t()
            loss_hist = loss_hist[:, self.inv]
        lh = loss_hist.cpu().numpy()
        ev = self.eval_hist[:R].cpu().numpy()
        ph = self.p_hist[:R].cpu() if self.mixture is not None else None
        train_loss, test_loss, test_acc = torch.zeros(self.R), torch.zeros(self.R), torch.zeros(self.R)
        for t in range(R):
            pt = ph[t] if ph is not None else self.p_all
            if self.scaffold:              # sum_S (q_k / server_lr) * loss_k, ascending client id
                S = np.arange(self.N) if self.sched is None else self.sched[t]
                train_loss[t] = torch.sum(self.sc_w[t] * torch.tensor([float(v) for v in lh[t][S]]))
            elif self.sched is not None:   # the sampled clients' weights and losses, ascending client id
                train_loss[t] = torch.sum(self.q_host[t] * torch.tensor([float(v) for v in lh[t][self.sched[t]]]))
            else:
                train_loss[t] = torch.sum(pt * torch.tensor([float(v) for v in lh[t]]))   # tools.py:344 / 434
            test_loss[t], test_acc[t] = float(ev[t, 0]), float(ev[t, 1])
            if self.verbose and self.rank == 0:
                print('Test loss: {}, \t Test Acc: {}'.format(float(ev[t, 0]), float(ev[t, 1])))
        if self.stats is not None:
            self.stats.update(W_global=self.W_g[:, :D].detach().clone(), N=self.N, local_clients=len(self.mine),
                              ld=self.ld)
            if self.W_hist is not None:
                self.stats['W_rounds'] = self.W_hist[:R, :, :D].cpu().numpy()
            if self.scaffold:
                self.stats['c_global'] = self.c_var[:, :D].detach().clone()
                if self.c_hist is not None:
                    self.stats['c_rounds'] = self.c_hist[:R, :, :D].cpu().numpy()
            if self.fedopt:
                self.stats['server_m'] = self.opt_m[:, :D].detach().clone()
                self.stats['server_v'] = self.opt_v[:, :D].detach().clone()
                if self.m_hist is not None:
                    self.stats['server_m_rounds'] = self.m_hist[:R, :, :D].cpu().numpy()
                    self.stats['server_v_rounds'] = self.v_hist[:R, :, :D].cpu().numpy()
            if self.qffl:
                self.stats['client_loss'] = self.qf_F[:R, :, 0].cpu().numpy()
                nh = self.qf_n[:R].cpu().numpy()
                norms = np.full((R, self.N), np.nan)
                for t in range(R):
                    S = np.arange(self.N) if self.sched is None else self.sched[t]
                    norms[t, S] = nh[t, :len(S)]
                self.stats['update_norms'] = norms
                self.stats['qffl_coef'] = self.qf_hc[:R].cpu().numpy()
            if self.robust:
                self.stats['trim_count'] = np.asarray(self.rb_b[:R], dtype=np.int64)
                if self.byz is not None:
                    self.stats['byzantine_ids'] = self.byz[0].copy()
            if self.krum:
                self.stats['krum_f'] = np.asarray([f for f, _ in self.kr_fm[:R]], dtype=np.int64)
                pk, sh = self.kr_pick[:R].cpu().numpy(), self.kr_score[:R].cpu().numpy()
                self.stats['krum_selected'] = [np.sort(pk[t, :self.kr_fm[t][1]].astype(np.int64)) for t in range(R)]
                scores = np.full((R, self.N), np.nan)
                for t in range(R):
                    S = np.arange(self.N) if self.sched is None else self.sched[t]
                    scores[t, S] = sh[t, :len(S)]
                self.stats['krum_scores'] = scores
                if self.byz is not None:
                    self.stats['byzantine_ids'] = self.byz[0].copy()
            if self.rfa:
                bh, dh = self.rf_b[:R].cpu().numpy().astype(np.float64), self.rf_dist[:R].cpu().numpy()
                wts, dst = np.full((R, self.N), np.nan), np.full((R, self.N), np.nan)
                for t in range(R):
                    S = np.arange(self.N) if self.sched is None else self.sched[t]
                    wts[t, S], dst[t, S] = bh[t, :len(S)], dh[t, :len(S)]
                self.stats['rfa_weights'], self.stats['rfa_dist'] = wts, dst
                self.stats['rfa_objective'] = self.rf_obj[:R].cpu().numpy()
                if self.byz is not None:
                    self.stats['byzantine_ids'] = self.byz[0].copy()
            if self.topk:
                # (a row whose threshold is 0 keeps its padding columns too: they are no parameters)
                th, kh = self.tk_tau[:R].cpu().numpy().astype(np.float64), self.tk_kept[:R].cpu().numpy()
                kept, tau = np.full((R, self.N), np.nan), np.full((R, self.N), np.nan)
                up, dense = np.zeros(R, np.int64), np.zeros(R, np.int64)
                for t in range(R):
                    S = np.arange(self.N) if self.sched is None else self.sched[t]
                    kept[t, S] = np.minimum(kh[t, :len(S)], self.C * D)
                    tau[t, S] = th[t, :len(S)]
                    up[t], dense[t] = int(np.sum(kept[t, S])), len(S) * self.C * D
                self.stats['topk_kept'], self.stats['topk_tau'] = kept, tau
                self.stats['uplink_values'], self.stats['uplink_dense'] = up, dense
                self.stats['residual_norm'] = self.tk_rnorm[:R].cpu().numpy()
                if self.tk_e is not None:
                    self.stats['residual'] = self.tk_e[:, :, :D].detach().clone()
            if self.dp:
                sh, rh = self.dp_state[:R].cpu().numpy(), self.dp_r[:R].cpu().numpy()
                norms = np.full((R, self.N), np.nan)
                for t in range(R):
                    S = np.arange(self.N) if self.sched is None else self.sched[t]
                    norms[t, S] = rh[t, :len(S)]
                self.stats['dp_clip'], self.stats['dp_sigma'] = sh[:, 0].copy(), sh[:, 1].copy()
                self.stats['dp_clipped'] = np.array([(self.N if self.sched is None else len(self.sched[t]))
                                                     for t in range(R)], np.float64) - sh[:, 2] - sh[:, 3]
                self.stats['dp_dropped'] = sh[:, 3].copy()
                self.stats['dp_norms'] = norms
                if self.byz is not None:
                    self.stats['byzantine_ids'] = self.byz[0].copy()
            if self.mixture is not None:
                p = self.mixture.p[self.pos_dev] if self.zshard else self.mixture.p
                self.stats['p'] = p.detach().clone()
            if self.sched is not None:
                self.stats['participants'] = [S.copy() for S in self.sched]
            for which, (_, hist, _) in self.client_eval.items():
                hist = self._mask_unsampled(hist)
                if self.sharded:      # as loss_hist: rank-major rows, then the caller's client order
                    hist = dist.allgather_rows(hist.permute(1, 0, 2).contiguous(), [len(s) for s in self.shards])
                    hist = hist[self.inv].permute(1, 0, 2)
                _client_eval_stats(self.stats, which, hist)
            for which, hist in self.local_hist.items():
                if which == 'own':
                    hist = self._mask_unsampled(hist)
                if self.sharded:      # each rank scored its own shard: gather, then the caller's client order
                    hist = dist.allgather_rows(hist.permute(1, 0, 2).contiguous(), [len(s) for s in self.shards])
                    hist = hist[self.inv].permute(1, 0, 2)
                _local_eval_stats(self.stats, which, hist, self.ns)
        return train_loss, test_loss, test_acc


def Scaffold(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
             batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, server_lr=1.0,
             weighting='size', stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """SCAFFOLD (Karimireddy et al., ICML 2020, option II; not in the reference): FedAvg's positional
    list, clients always parallel.  Every local step adds d = c - c_i to the gradient, every trained
    client leaves c_i+ = c_i - c + (x - y_i) / (K_i lr) behind (fs_local_train_scaffold), and the
    server folds the sampled models twice from one pass (fs_aggregate_scaffold):
    x += server_lr * sum_S (p_k / sum_S p) (y_k - x) and c = (1 - sum_S p) c + sum_S p_k (x - y_k) / (K_k lr),
    which keeps c = sum_j p_j c_j over all clients.  ``weighting='size'``: p_i = n_i / n (the project's
    convention); ``'uniform'``: p_i = 1 / N, the paper's Algorithm 1 literally.  The global generator
    is consumed exactly as by ``FedAvg(clients='parallel')`` with the same ``participation``;
    ``train_loss[t] = sum_S (p_k / sum_S p) loss_k``.  ``stats['c_global']`` [C, D]; with
    ``stats['trace']`` also ``stats['c_rounds']`` [R, C, D].  ValueError for ``prox=True``,
    ``type='regression'`` and ``batch_size > 64``; NotImplementedError over more than one
    torch.distributed rank.  ``mu`` is ignored."""
    _check_scaffold(type, prox, batch_size, weighting, server_lr)
    return _run('scaffold', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                False, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed, server_lr=server_lr,
                weighting=weighting)


def _run(algo, *args, stats=None, verbose=True, options=None, participation=None, sample_seed=0, **kw):
    fed = Federation(algo, *args, stats=stats, verbose=verbose, options=options, participation=participation,
                     sample_seed=sample_seed, **kw)
    for _ in range(fed.R):
        fed.round()
    return fed.results()


def FedAvg(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
           batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *,
           clients='sequential', stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """tools.py:329-353.  ``options``: launch-scheduling options (``OPTIONS``).  ``participation`` /
    ``sample_seed``: partial client participation (module docstring; needs ``clients='parallel'``)."""
    return _run('fedavg', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, clients, stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed)


def FedProx(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=True, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *,
            clients='sequential', stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """tools.py:356-380 (FedAvg with the proximal term on by default).  ``participation`` /
    ``sample_seed`` as FedAvg's."""
    return _run('fedprox', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, clients, stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed)


def FedNova(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *,
            clients='sequential', variant='reference', stats=None, verbose=True, options=None, participation=None,
            sample_seed=0):
    """tools.py:383-410: FedAvg's round with FedNova's aggregate (fs_aggregate_nova).
    ``variant='reference'`` reproduces the reference's lines 401-405, which scale the clients'
    WEIGHTS by p_j*Tau_eff/Tau_j with Tau_j = n_j*E/B: for unequal client sizes those coefficients
    sum to N*sum_j p_j^2 > 1, very likely why exp.py leaves the call commented out.
    ``variant='updates'`` is the method of Wang et al. (2020): W_g + sum_j a_j (W_j - W_g) with
    a_j = p_j*tau_eff/tau_j over the steps tau_j = E*ceil(n_j/B) each client really took; it needs
    ``clients='parallel'``.  train_loss uses the plain p in both (tools.py:400).  ``participation`` /
    ``sample_seed`` as FedAvg's, the coefficients taken over each round's sample."""
    _check_nova(variant, clients)
    return _run('fednova', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, clients, stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed, variant=variant)


def FedOpt(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
           batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, server_opt='adam',
           server_lr=None, beta1=0.9, beta2=0.99, tau=1e-3, v0=None, stats=None, verbose=True, options=None,
           participation=None, sample_seed=0):
    """Adaptive federated optimization (Reddi et al., ICLR 2021, Algorithm 2) and server momentum
    (FedAvgM, Hsu et al. 2019); not in the reference.  FedAvg's positional list, clients always
    parallel.  Local training is FedAvg's launch unchanged -- both tasks, ``prox=True``, any
    ``batch_size`` the task's trainer accepts, ``participation`` -- and only the server step differs
    (fs_aggregate_opt): with delta = sum_S (p_k / sum_S p) (W_k - x),
    ``'avgm'``: m = beta1 m + delta, x += server_lr m;  the others m = beta1 m + (1 - beta1) delta,
    ``'adagrad'``: v += delta^2;  ``'adam'``: v = beta2 v + (1 - beta2) delta^2;
    ``'yogi'``: v -= (1 - beta2) delta^2 sign(v - delta^2);  x += server_lr m / (sqrt(v) + tau),
    without bias correction, as the paper.  m0 = 0 and ``v0=None`` means tau^2 (the paper's
    initialisation).  ``server_lr=None`` takes the rule's default (``SERVER_LR_DEFAULT``: 1 for
    'avgm'; 0.1 for the adaptive rules, a point of the paper's grid -- a default, not a tuned value).
    The host scalars are ``server_opt_scalars``'.  The global generator is consumed exactly as by
    ``FedAvg(clients='parallel')`` with the same ``participation``, and ``train_loss`` is FedAvg's.
    ``stats['server_m']`` / ``stats['server_v']`` [C, D]; with ``stats['trace']`` also
    ``stats['server_m_rounds']`` / ``stats['server_v_rounds']`` [R, C, D] next to ``W_rounds``.
    ValueError for an unknown rule, ``tau <= 0``, a beta outside [0, 1) and ``server_lr <= 0``;
    NotImplementedError over more than one torch.distributed rank."""
    _check_server_opt(server_opt, server_lr, beta1, beta2, tau)
    return _run('fedopt', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed,
                server_opt=dict(rule=server_opt, server_lr=server_lr, beta1=beta1, beta2=beta2, tau=tau, v0=v0))


def FedAvgM(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, server_lr=1.0,
            beta1=0.9, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """``FedOpt(server_opt='avgm')``: server momentum ``beta1``, m = beta1 m + delta, x += server_lr m."""
    return FedOpt(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                  lambda_reg_if, lambda_reg, round, server_opt='avgm', server_lr=server_lr, beta1=beta1, stats=stats,
                  verbose=verbose, options=options, participation=participation, sample_seed=sample_seed)


def _adaptive(rule):
    def f(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
          batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *,
          server_lr=SERVER_LR_DEFAULT[rule], beta1=0.9, beta2=0.99, tau=1e-3, v0=None, stats=None, verbose=True,
          options=None, participation=None, sample_seed=0):
        return FedOpt(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                      lambda_reg_if, lambda_reg, round, server_opt=rule, server_lr=server_lr, beta1=beta1, beta2=beta2,
                      tau=tau, v0=v0, stats=stats, verbose=verbose, options=options, participation=participation,
                      sample_seed=sample_seed)
    f.__name__ = f.__qualname__ = 'Fed' + rule.capitalize()
    f.__doc__ = ("``FedOpt(server_opt=%r)`` (Reddi et al., ICLR 2021).  ``server_lr`` defaults to 0.1, a point of the "
                 "paper's grid: a default, not a tuned value (``beta2`` is unused by 'adagrad')." % rule)
    return f


FedAdagrad, FedAdam, FedYogi = _adaptive('adagrad'), _adaptive('adam'), _adaptive('yogi')


def QFedAvg(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, q=1.0,
            weighting='size', lipschitz=None, stats=None, verbose=True, options=None, participation=None,
            sample_seed=0):
    """q-FedAvg (q-FFL; Li, Sanjabi, Beirami, Smith, ICLR 2020; not in the reference): FedAvg's positional
    list, clients always parallel.  Local training is FedAvg's launch unchanged -- both tasks,
    ``prox=True``, any ``batch_size`` the task's trainer accepts, ``participation`` -- and only the server
    step differs.  With x the round's starting model, F_k its loss on client k's own rows (mean
    cross-entropy or MSE, ``LocalEvaluator``), Ft = F_k + 1e-10, L the Lipschitz estimate
    (``lipschitz``; None: 1 / lr_t with the round's decayed learning rate) and S the sampled clients:
    u_k = p_k Ft^q,  g_k = p_k q Ft^(q-1) L^2  (fs_qffl_coef);
    x' = x + (L / H) sum_S u_k (W_k - x),  H = L sum_S u_k + sum_S g_k ||W_k - x||^2  (fs_aggregate_qffl,
    the fold and the norms from one pass) -- the paper's w - sum Delta_k / sum h_k.
    ``weighting='size'``: p_k = n_k / n; ``'uniform'``: p_k = 1 / N; over all N clients, not renormalised
    over the sample (H normalises), so ``q=0`` is FedAvg over the sample.  A round enqueues, on one
    stream: the local evaluation of x, fs_qffl_coef, FedAvg's TRAIN, AGGREGATE and EVAL.  Under
    ``participation`` the evaluation still scores all N clients (fs_eval_clients has no subset form)
    and the sample is uniform as FedAvg's (not the paper's sampling by p_k).  The global generator
    is consumed exactly as by ``FedAvg(clients='parallel')`` with the same ``participation``, and
    ``train_loss`` is FedAvg's.  ``stats['client_loss']`` [R, N] float64 (the F_k of each round's
    starting model), ``stats['update_norms']`` [R, N] (||W_k - x||^2, NaN where a client was not sampled),
    ``stats['qffl_coef']`` [R, 2] (H and coef = f32(L / H)).  ValueError for ``q < 0``, ``lipschitz <= 0``
    and an unknown ``weighting``; NotImplementedError over more than one torch.distributed rank."""
    _check_qffl(q, weighting, lipschitz)
    return _run('qfedavg', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed, weighting=weighting,
                qffl=dict(q=q, lipschitz=lipschitz))


def FedRobust(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
              batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, rule='median',
              trim=0.1, byzantine=None, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """Robust aggregation (Yin, Chen, Ramchandran, Bartlett, ICML 2018; not in the reference): FedAvg's
    positional list, clients always parallel.  Local training is FedAvg's launch unchanged -- both
    tasks, ``prox=True``, any ``batch_size`` the task's trainer accepts, ``participation`` -- and the server
    step is fs_aggregate_robust: per parameter, over the round's M clients, the b smallest and b largest
    values are dropped and the rest averaged, unweighted.  ``rule='median'``: b = (M - 1) // 2;
    ``'trimmed_mean'``: b = floor(trim * M), clamped so that 2b < M; ``'mean'``: b = 0, the uniform
    mean (no protection: the baseline an attack is shown against).  Up to b clients per side may
    return arbitrary bits, NaN and Inf included.  ``byzantine=dict(ids=... | fraction=f, attack='sign_flip'
    | 'gaussian' | 'nan', scale=1.0, seed=0)`` makes those clients misbehave: their rows of the
    clients x params buffer are overwritten between TRAIN and AGGREGATE in the rounds that sample
    them, with W_g - scale (W_k - W_g), W_g + scale N(0, 1) (``byzantine_noise(seed, t, ...)``) or NaN;
    with ``fraction`` the ids are fixed once from ``seed``.  The global generator is consumed exactly
    as by ``FedAvg(clients='parallel')`` with the same ``participation``, and ``train_loss`` is FedAvg's
    (the clients' own training losses, the corrupted ones' included).  ``stats['trim_count']`` [R] int64,
    ``stats['byzantine_ids']`` the corrupted ids.  ValueError for ``trim`` outside [0, 0.5), an unknown
    ``rule``, a bad ``byzantine`` or a round whose M is 0 or above ``engine.robust_max_m()``;
    NotImplementedError over more than one torch.distributed rank."""
    _check_robust(rule, trim)
    byzantine_plan(len(y_train), byzantine)
    return _run('fedrobust', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed,
                robust=dict(rule=rule, trim=trim, byzantine=byzantine))


def FedMedian(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
              batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, byzantine=None,
              stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """``FedRobust(rule='median')``: the coordinate-wise median of the round's clients."""
    return FedRobust(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                     lambda_reg_if, lambda_reg, round, rule='median', byzantine=byzantine, stats=stats,
                     verbose=verbose, options=options, participation=participation, sample_seed=sample_seed)


def FedTrimmedMean(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
                   batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, trim=0.1,
                   byzantine=None, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """``FedRobust(rule='trimmed_mean')``: the coordinate-wise ``trim``-trimmed mean of the round's clients."""
    return FedRobust(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                     lambda_reg_if, lambda_reg, round, rule='trimmed_mean', trim=trim, byzantine=byzantine,
                     stats=stats, verbose=verbose, options=options, participation=participation,
                     sample_seed=sample_seed)


def FedKrum(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, f=0.1, m=None,
            byzantine=None, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """Krum and Multi-Krum (Blanchard, El Mhamdi, Guerraoui, Stainer, NeurIPS 2017; not in the reference):
    FedAvg's positional list, clients always parallel.  Local training is FedAvg's launch unchanged -- both
    tasks, ``prox=True``, any ``batch_size`` the task's trainer accepts, ``participation`` -- and the server
    step is fs_aggregate_krum: the squared distances between the round's M updates W_k - W_g, every
    client's score (the sum of its M - f - 2 smallest distances), and the unweighted mean of the m clients
    with the smallest (score, id).  ``f``: the number of clients that may return arbitrary bits, an int
    count or a fraction in [0, 0.5) (floor(f * M) of the round's own M); ``m``: None for M - f (the
    one-shot Multi-Krum), 1 for Krum, or a count.  ``byzantine=`` as in ``FedRobust``.  The global generator
    is consumed exactly as by ``FedAvg(clients='parallel')`` with the same ``participation``, and
    ``train_loss`` is FedAvg's.  ``stats['krum_f']`` [R] int64, ``stats['krum_selected']`` R sorted id arrays,
    ``stats['krum_scores']`` [R, N] float64 (NaN where a client was not sampled), ``stats['byzantine_ids']``.
    ValueError for a bad ``f`` or ``m``, a bad ``byzantine``, a round with M < 2f + 3 or m > M - f, or M above
    ``engine.krum_max_m()``; NotImplementedError over more than one torch.distributed rank."""
    _check_krum(f, m)
    byzantine_plan(len(y_train), byzantine)
    if participation is None:
        krum_counts(f, m, len(y_train))
    return _run('fedkrum', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed,
                krum=dict(f=f, m=m, byzantine=byzantine))


def Krum(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
         batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, f=0.1, byzantine=None,
         stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """``FedKrum(m=1)``: the one client whose update lies closest to its M - f - 2 nearest neighbours."""
    return FedKrum(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                   lambda_reg_if, lambda_reg, round, f=f, m=1, byzantine=byzantine, stats=stats, verbose=verbose,
                   options=options, participation=participation, sample_seed=sample_seed)


def MultiKrum(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
              batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, f=0.1,
              byzantine=None, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """``FedKrum(m=None)``: the mean of the M - f clients with the smallest scores."""
    return FedKrum(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
                   lambda_reg_if, lambda_reg, round, f=f, m=None, byzantine=byzantine, stats=stats, verbose=verbose,
                   options=options, participation=participation, sample_seed=sample_seed)


def FedRFA(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
           batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, iters=3, nu=1e-6,
           init='start', weighting='size', byzantine=None, stats=None, verbose=True, options=None, participation=None,
           sample_seed=0):
    """RFA (Pillutla, Kakade, Harchaoui, IEEE TSP 2022; not in the reference): FedAvg's positional list,
    clients always parallel.  Local training is FedAvg's launch unchanged -- both tasks, ``prox=True``, any
    ``batch_size`` the task's trainer accepts, ``participation`` -- and the server step is fs_aggregate_rfa:
    ``iters`` smoothed Weiszfeld iterations towards the geometric median of the round's M models under the
    weights p_k (``weighting='size'``: the round's FedAvg weights; ``'uniform'``: 1 / M), each one distance
    pass and one fold with the weights p_k / max(nu, ||W_k - v||); a row that is not finite weighs 0.
    ``init='start'`` iterates from the round-start model, ``'mean'`` from the finite rows' weighted mean as
    the paper does -- which one finite row of huge norm drags far out at small ``iters``: it is offered for
    fidelity and carries no robustness claim.  ``byzantine=`` as in ``FedRobust``.  The global generator is
    consumed exactly as by ``FedAvg(clients='parallel')`` with the same ``participation``, and ``train_loss``
    is FedAvg's.  ``stats['rfa_weights']`` [R, N] float64 (the last weights used; NaN where a client was not
    sampled), ``stats['rfa_dist']`` [R, N] (the distances to the new global model), ``stats['rfa_objective']``
    [R, iters + 2] and ``stats['byzantine_ids']``.  ValueError for a bad ``iters``, ``nu``, ``init``,
    ``weighting`` or ``byzantine``, or a round with M = 0 or M above ``engine.rfa_max_m()``;
    NotImplementedError over more than one torch.distributed rank."""
    _check_rfa(iters, nu, init, weighting)
    byzantine_plan(len(y_train), byzantine)
    return _run('fedrfa', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed, weighting=weighting,
                rfa=dict(iters=iters, nu=nu, init=init, byzantine=byzantine))


def FedTopK(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
            batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, ratio=0.01,
            error_feedback=True, stats=None, verbose=True, options=None, participation=None, sample_seed=0):
    """Top-k sparsified uploads with error feedback (Aji & Heafield 2017; Stich, Cordonnier & Jaggi, NeurIPS
    2018; Sattler et al. 2019; not in the reference): FedAvg's positional list, clients always parallel.
    Local training is FedAvg's launch unchanged -- both tasks, ``prox=True``, any ``batch_size`` the task's
    trainer accepts, ``participation`` -- and the server step is fs_aggregate_topk: every sampled client's
    corrected update a_k = (W_k - W_g) + e_k is cut to the entries whose magnitude is at or above its
    k-th largest, k = ``topk_count(ratio, C, D)`` (ties at the threshold are all kept, so a client may send
    more than k values), the kept parts are folded onto ``W_g`` with FedAvg's weights p_k / sum_S p, and what
    was not sent stays in the client's residual e_k for its next round.  ``error_feedback=False``: no
    residual, the rest is dropped -- the variant known to stall under non-IID data.  The residual of a
    client that sits a round out is carried unchanged.  Selection is by magnitude bits, so a NaN or an
    Inf in an update is always transmitted: the rule carries no robustness claim.  ``ratio=1.0`` is
    ``FedAvgM(server_lr=1.0, beta1=0.0)`` bit for bit.  The global generator is consumed exactly as by
    ``FedAvg(clients='parallel')`` with the same ``participation``, and ``train_loss`` is FedAvg's.
    ``stats['topk_kept']`` [R, N] float64 (the values each client sent; NaN where it was not sampled),
    ``stats['topk_tau']`` [R, N] (its threshold magnitude), ``stats['uplink_values']`` [R] int64 (their
    sum), ``stats['uplink_dense']`` [R] (M * C * D), ``stats['residual_norm']`` [R] (the norm of all
    residuals after the round; 0 without memory) and ``stats['residual']`` [N, C, D] (with memory).
    ValueError for a bad ``ratio`` or ``error_feedback``; NotImplementedError over more than one
    torch.distributed rank."""
    _check_topk(ratio, error_feedback)
    topk_count(ratio, num_classes, D)
    return _run('fedtopk', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed,
                topk=dict(ratio=ratio, error_feedback=error_feedback))


def DPFedAvg(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01, epoch=2,
             batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, round=100, *, clip=1.0,
             noise_multiplier=1.0, noise_seed=0, weighting='uniform', adaptive=None, byzantine=None, stats=None,
             verbose=True, options=None, participation=None, sample_seed=0):
    """DP-FedAvg: user-level differential privacy by per-client norm clipping and Gaussian noise on the aggregate
    (McMahan, Ramage, Talwar & Zhang, ICLR 2018; Geyer, Klein & Nabi 2017; not in the reference): FedAvg's
    positional list, clients always parallel.  Local training is FedAvg's launch unchanged -- both tasks,
    ``prox=True``, any ``batch_size`` the task's trainer accepts, ``participation`` -- and the server step is
    fs_aggregate_dp: every sampled client's update W_k - W_g is scaled to a norm of at most ``clip`` (S), the
    clipped updates are folded onto ``W_g`` with the weights q_k (``weighting='uniform'``: 1 / M, the
    fixed-denominator estimator; ``'size'``: FedAvg's p_k / sum_S p), and Gaussian noise of standard deviation
    ``noise_multiplier * clip * max_k q_k`` is added from a counter-based generator on the device
    (Philox4x32-10 keyed by ``noise_seed``, counted by round and position: the same bits on every run).  An
    update whose norm is not finite (it holds a NaN or an Inf, or its squares overflow) is dropped and counted.
    ``clip=inf, noise_multiplier=0`` is ``FedAvgM(server_lr=1.0, beta1=0.0)`` bit for bit (size weighting).
    ``adaptive=dict(quantile=, lr=, count_noise=)``: the clip follows the ``quantile`` of the update norms
    (Andrew, Thakkar, McMahan & Ramaswamy, NeurIPS 2021), S <- S exp(-lr ((b + count_noise g) / M - quantile))
    with b the number of unclipped updates, on the device; the noise of a round uses that round's S.
    ``byzantine=``: as ``FedRFA``'s -- norm clipping bounds one client's influence (Sun et al. 2019).
    This is a simulator: the noise is floating-point Gaussian with a truncated tail (|g| < 6.77), not a deployed
    mechanism's, and NO PRIVACY ACCOUNTANT is provided.  ``participation`` samples a fixed-size subset without
    replacement, to which the Poisson-subsampled RDP bounds do not apply as they stand; the stats carry what an
    external accountant needs (the noise multiplier, M_t / N, the rounds).  The global generator is consumed
    exactly as by ``FedAvg(clients='parallel')`` with the same ``participation``, and ``train_loss`` is FedAvg's.
    Stats, float64 on the CPU: ``stats['dp_clip']`` [R] (the round's S), ``stats['dp_sigma']`` [R],
    ``stats['dp_norms']`` [R, N] (the update norms; NaN where a client was not sampled), ``stats['dp_clipped']``
    [R] (updates scaled down) and ``stats['dp_dropped']`` [R].  ValueError for a bad keyword;
    NotImplementedError over more than one torch.distributed rank."""
    _check_dp(clip, noise_multiplier, noise_seed, weighting, adaptive)
    byzantine_plan(len(y_train), byzantine)
    return _run('dpfedavg', X_train, y_train, X_test, y_test, None, type, num_classes, D, lr, epoch, batch_size,
                prox, mu, lambda_reg_if, lambda_reg, round, None, 'parallel', stats=stats, verbose=verbose,
                options=options, participation=participation, sample_seed=sample_seed, weighting=weighting,
                dp=dict(clip=clip, noise_multiplier=noise_multiplier, noise_seed=noise_seed, adaptive=adaptive,
                        byzantine=byzantine))


def FedAMW(X_train, y_train, X_test, y_test, validloader, type='classification', num_classes=10, D=200, lr=0.01,
           epoch=2, batch_size=32, prox=False, mu=0.1, lambda_reg_if=True, lambda_reg=0.01, round=100, lr_p=5e-5,
           *, clients='sequential', stats=None, verbose=True, options=None):
    """tools.py:413-463: FedAvg-style round + learned mixture weights p (SGD momentum 0.9
    on the pooled validation set, ``round`` inner epochs per round), aggregate with p."""
    return _run('fedamw', X_train, y_train, X_test, y_test, validloader, type, num_classes, D, lr, epoch,
                batch_size, prox, mu, lambda_reg_if, lambda_reg, round, lr_p, clients, stats=stats, verbose=verbose,
                options=options)


# --------------------------------------------------------------------------- #
# Random Fourier features (tools.py:15-31)
# --------------------------------------------------------------------------- #
def RFF(d, sigma, D):
    """tools.py:15-19: W ~ N(0, sigma) [d, D], b ~ U(0, 2 pi) [1, D], drawn on torch's global
    CPU generator exactly as the reference draws them (Uniform.sample((1, D)) -> (1, D, 1) ->
    view), then placed on the GPU.

    RNG stream: this reproduces the reference run on a CPU-only host (device = cpu,
    tools.py:12), which is what the golden fixtures pin.  On a CUDA/ROCm host the reference
    draws W and b from the GPU generator instead and leaves the CPU stream untouched, so its
    later MLP inits and DataLoader shuffles are shifted by these d*D + D draws relative to
    this drop-in; that GPU-host stream is not reproduced (parity unpinned for it)."""
    m = torch.distributions.Uniform(torch.tensor([0.0]), torch.tensor([2 * torch.pi]))
    W = torch.normal(0, sigma, size=(d, D))
    b = m.sample((1, D)).view(-1, D)
    dev = _device()
    return W.to(dev), b.to(dev)


def feature_mapping(X_train, X_test, k_par=10, D=200, type='gaussian'):
    """tools.py:22-31: one RFF draw, then ``1/sqrt(D) * cos(X W + b)`` for every slice of
    ``X_train`` ([P, n, d]; exp.py:63 passes P = 1) and for ``X_test`` -- each map one
    fs_feature_map launch (MFMA GEMM with the cos epilogue fused).  Returns GPU tensors
    [P, n, D] and [n_t, D]; other ``type`` values return the inputs unchanged."""
    if type != 'gaussian':
        return X_train, X_test
    X_train = torch.as_tensor(X_train)
    W, b = RFF(X_train[0].shape[1], k_par, D)
    out = torch.empty(X_train.shape[0], X_train.shape[1], D, device=W.device, dtype=torch.float32)
    for i in range(len(X_train)):
        engine.feature_map(X_train[i], W, b, D, out=out[i])
    return out, engine.feature_map(X_test, W, b, D)


# --------------------------------------------------------------------------- #
# Single-shot algorithms (tools.py:240-326)
# --------------------------------------------------------------------------- #
def _chain_train(X_train, y_train, W_init, D, C, lr, epoch, batch_size, prox, mu, reg, lam, dev, loss='ce'):
    """One shared model trained by the clients in turn (tools.py:263-266 / 284-287: train_loop
    mutates the one ``model``), each for ``epoch`` epochs and anchored (prox) to its start --
    one fs_local_train launch in chained mode.  Consumes the generator like the reference
    (epoch passes per client, client-major).  Returns (feats, W_out [N, C, ld], loss [N])."""
    feats = engine.Features([torch.as_tensor(x) for x in X_train], [torch.as_tensor(y) for y in y_train], D, dev,
                            float_targets=loss == 'mse')
    trainer = engine.LocalTrainer(feats, C, batch_size, epoch, chained=True, prox=prox, loss=loss)
    trainer.upload_perms(rng.draw_pass_seeds(trainer.N * epoch))
    W0 = torch.zeros(C, feats.ld, device=dev, dtype=torch.float32)
    W0[:, :D].copy_(W_init)
    W_out, loss = trainer.run(W0, lr, prox, mu, reg, lam, chained=True)
    return feats, trainer, W_out, loss


def _test(evaluator, W, out2):
    rng.draw_pass_seeds(1)                  # test_loop's shuffled pass (tools.py:219-220)
    evaluator.run(W, out2)


def _print_tests(ev, verbose):
    if verbose and dist.world()[0] == 0:
        for tl, ta in ev:
            print('Test loss: {}, \t Test Acc: {}'.format(float(tl), float(ta)))


def Centralized(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01,
                epoch=200, batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, *,
                stats=None, verbose=True):
    """tools.py:240-255: every client's rows concatenated (client order), ONE train_loop of
    ``epoch`` epochs (exp.py:116 passes local_epoch * Round), one test_loop.  Returns
    (train_loss, test_loss, test_acc) as Python floats, like the reference's Meter averages."""
    _check_inputs(type, X_train, y_train, num_classes, batch_size, epoch, 0, y_test)
    if _local_eval_request(stats):
        raise ValueError("stats['local_eval'] has no meaning for Centralized: the clients' rows are pooled into one "
                         "client, so there are no per-client rows to score on")
    dev = _device()
    C = int(num_classes)
    W_init = init_weights(D, C)
    Xc = torch.cat([torch.as_tensor(x).to(dev, torch.float32) for x in X_train], 0)
    task = _loss_of(type)
    yc = torch.cat([torch.as_tensor(y).reshape(-1).to('cpu', torch.float32 if task == 'mse' else torch.int64)
                    for y in y_train], 0)
    feats, trainer, W_out, loss = _chain_train([Xc], [yc], W_init, D, C, lr, epoch, batch_size, prox, mu,
                                               lambda_reg_if, lambda_reg, dev, loss=task)
    ev = engine.Evaluator(X_test, y_test, D, C, dev, feats.ld, loss=task)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    _test(ev, W_out[0], out2)
    trainer.check_errors()
    res = out2.cpu().numpy()
    _print_tests([res], verbose)
    if stats is not None:
        stats.update(W_global=W_out[0, :, :D].detach().clone())
    return float(loss[0].item()), float(res[0]), float(res[1])


def Distributed(X_train, y_train, X_test, y_test, type='classification', num_classes=10, D=200, lr=0.01,
                epoch=200, batch_size=32, prox=False, mu=0.1, lambda_reg_if=False, lambda_reg=0.01, *,
                stats=None, verbose=True):
    """tools.py:258-276: chained local training of ``epoch`` epochs per client, one
    n_j-weighted aggregate (fs_aggregate, the reference's left fold), one test_loop.  Returns
    (train_loss 0-dim fp32 tensor, test_loss float, test_acc float)."""
    _check_inputs(type, X_train, y_train, num_classes, batch_size, epoch, 0, y_test)
    client_eval = _client_eval_request(stats, False)
    local_eval = _local_eval_request(stats)
    dev = _device()
    C = int(num_classes)
    W_init = init_weights(D, C)
    ns = np.array([len(y) for y in y_train])
    p = torch.tensor(ns / sum(ns), dtype=torch.float32)
    task = _loss_of(type)
    feats, trainer, W_out, loss = _chain_train(X_train, y_train, W_init, D, C, lr, epoch, batch_size, prox, mu,
                                               lambda_reg_if, lambda_reg, dev, loss=task)
    ld = feats.ld
    agg = engine.Aggregator(len(ns), C, ld, dev, chunks=1)
    W_g = torch.empty(C, ld, device=dev, dtype=torch.float32)
    agg.run(W_out, p.to(dev), W_g)
    ev = engine.Evaluator(X_test, y_test, D, C, dev, ld, loss=task)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    _test(ev, W_g, out2)
    trainer.check_errors()
    res = out2.cpu().numpy()
    train_loss = torch.sum(p * torch.tensor([float(v) for v in loss.cpu().numpy()]))    # tools.py:268
    _print_tests([res], verbose)
    if stats is not None:
        stats.update(W_global=W_g[:, :D].detach().clone())
    if 'test' in client_eval:
        _client_eval_once(stats, 'test', ev.f, C, len(ns), task, W_out)
    if local_eval:
        le = engine.LocalEvaluator(feats, C, loss=task)
        if 'global' in local_eval:
            _local_eval_once(stats, 'global', le, W_g, 0)
        if 'own' in local_eval:
            _local_eval_once(stats, 'own', le, W_out, C * ld)
    return train_loss, float(res[0]), float(res[1])


def FedAMW_OneShot(X_train, y_train, X_test, y_test, validloader, type='classification', num_classes=10, D=200,
                   lr=0.01, epoch=200, batch_size=32, prox=False, mu=0.1, lambda_reg_if=True, lambda_reg=0.01,
                   round=100, lr_p=5e-5, *, stats=None, verbose=True):
    """tools.py:279-326: chained local training once (``epoch`` epochs per client), then
    ``round`` times: one pass of plain SGD (no momentum, tools.py:300) on the mixture weights
    over the validation loader, aggregate, test_loop.  Z = the stacked client models applied
    to the validation set is computed once (fs_mix_z; the stack is fixed, tools.py:293-297).

    The reference's aggregate compounds: ``global_weights = local_weights[0]``
    aliases client 0's state dict, so from round 1 on the fold starts from the previous
    global model: W(t) = W(t-1) * p0(t) + sum_{j>0} p_j(t) W_j (W(-1) = W_0).  Reproduced with
    two fs_aggregate launches per round (a 1-client fold scales W(t-1) by p0(t) into row 0 of
    a copy of the clients x params buffer; the N-client fold with weight 1 on that row adds
    the rest), bitwise the reference's sequence of roundings.
    Returns (train_loss 0-dim fp32 tensor, test_loss [round], test_acc [round])."""
    _check_inputs(type, X_train, y_train, num_classes, batch_size, epoch, round, y_test,
                  validloader.dataset.tensors[1])
    client_eval = _client_eval_request(stats, True)
    local_eval = _local_eval_request(stats)
    dev = _device()
    C, R = int(num_classes), int(round)
    W_init = init_weights(D, C)
    ns = np.array([len(y) for y in y_train])
    N = len(ns)
    p0 = torch.tensor(ns / np.sum(ns), dtype=torch.float32)
    task = _loss_of(type)
    feats, trainer, W_out, loss = _chain_train(X_train, y_train, W_init, D, C, lr, epoch, batch_size, prox, mu,
                                               lambda_reg_if, lambda_reg, dev, loss=task)
    ld = feats.ld
    Xv, yv = validloader.dataset.tensors[:2]
    if not isinstance(validloader.sampler, torch.utils.data.RandomSampler):
        raise NotImplementedError('validloader must shuffle (exp.py:99)')
    mix = engine.Mixture(Xv, yv, D, C, N, int(validloader.batch_size), p0, dev, ld, momentum=0.0, loss=task)
    ev = engine.Evaluator(X_test, y_test, D, C, dev, ld, loss=task)
    agg1 = engine.Aggregator(1, C, ld, dev, chunks=1)
    aggN = engine.Aggregator(N, C, ld, dev, chunks=1)
    W_agg = W_out.clone()                       # row 0 rewritten every round, rows 1.. = W_j
    W_prev = W_out[0].clone()
    q = torch.ones(N, dtype=torch.float32, device=dev)
    W_g = torch.empty(C, ld, device=dev, dtype=torch.float32)
    eval_hist = torch.empty(max(R, 1), 2, dtype=torch.float64, device=dev)
    p_hist = torch.empty(max(R, 1), N, dtype=torch.float32, device=dev)
    W_hist = torch.empty(R, C, ld, device=dev) if (stats is not None and stats.get('trace')) else None
    le = engine.LocalEvaluator(feats, C, loss=task) if local_eval else None
    lg_hist = torch.zeros(R, N, 2, dtype=torch.float64, device=dev) if 'global' in local_eval else None
    for t in range(R):
        seeds = rng.draw_pass_seeds(2)          # the validation pass, then test_loop's pass
        mix.solve(W_out, seeds[:1], lr_p, z=(t == 0))
        agg1.run(W_prev, mix.p, W_agg[0])       # W(t-1) * p0(t), in place in the reference
        if N > 1:
            q[1:].copy_(mix.p[1:])
        aggN.run(W_agg, q, W_g)
        W_prev.copy_(W_g)
        p_hist[t].copy_(mix.p)
        if W_hist is not None:
            W_hist[t].copy_(W_g)
        ev.run(W_g, eval_hist[t])
        if lg_hist is not None:
            le.run(W_g, 0, lg_hist[t])
    trainer.check_errors()
    mix.check_errors()
    train_loss = torch.sum(p0 * torch.tensor([float(v) for v in loss.cpu().numpy()]))   # tools.py:292
    evh = eval_hist[:R].cpu().numpy()
    _print_tests(evh, verbose)
    test_loss = torch.tensor(evh[:, 0], dtype=torch.float32) if R else torch.zeros(0)
    test_acc = torch.tensor(evh[:, 1], dtype=torch.float32) if R else torch.zeros(0)
    if stats is not None:
        stats.update(W_global=W_g[:, :D].detach().clone(), p=mix.p.detach().clone())
        if stats.get('trace'):
            stats['p_rounds'] = p_hist[:R].cpu().numpy()
            stats['W_rounds'] = W_hist[:, :, :D].cpu().numpy()
    if 'test' in client_eval:
        _client_eval_once(stats, 'test', ev.f, C, N, task, W_out)
    if 'val' in client_eval:      # the one Z of the p-solve (fs_mix_z ran in round 0), if there was a round
        _client_eval_once(stats, 'val', mix.f, C, N, task, W_out, Z=mix.Z if R else None)
    if lg_hist is not None:
        _local_eval_stats(stats, 'global', lg_hist, ns)
    if 'own' in local_eval:
        _local_eval_once(stats, 'own', le, W_out, C * ld)
    return train_loss, test_loss, test_acc
