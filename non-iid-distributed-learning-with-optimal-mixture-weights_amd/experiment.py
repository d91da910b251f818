"""The experiment driver -- counterpart of the reference's ``exp.py`` (exp.py:22-143), on MI355X.

    python run_experiment.py --dataset a9a --D 2000 --clients 10 --rounds 100 ...

Reproduces exp.py's sequence exactly, consuming torch's and numpy's global generators in
the same order:
  1. seeds: torch.manual_seed(100), np.random.seed(100)                       exp.py:28-29
  2. load + Dirichlet partition (numpy reseeded to 2020)                        exp.py:60, utils.py:320
  3. the full-batch train pass (2 draws + randperm) and test pass (1 draw)     exp.py:61-62
     -- the partition's indices then address the SHUFFLED training rows, as in the
     reference
  4. the RFF draw and feature map (fs_feature_map)                              exp.py:63
  5. data heterogeneity (fs_gram + fs_hetero)                                   exp.py:66-74
  6. per-client 20/80 validation split with np.random.shuffle                  exp.py:78-99
  7. Centralized, Distributed, FedAMW_OneShot, FedAvg, FedProx, FedAMW with exp.py's
     positional arguments                                                       exp.py:102-130
and writes ``{result_dir}/exp1_{dataset}.pkl`` with the reference's keys (epochs,
train_loss, test_loss, test_acc of shape (6, Round, n_repeats), heterogeneity, name).

Stated choices where the reference is silent or broken: datasets missing from
``get_parameter`` (a9a, covtype) fall to its default branch, which lacks ``lr_p``,
``lr_p_os`` and ``lambda_reg_os``: they default to 1e-3, 1e-3 and ``lambda_reg``
(SURVEY.md 8(d) config 1); LIBSVM files that are absent are synthesised in their shape
(functions/utils.py).  ``clients='parallel'`` (not the reference's semantics) runs FedAvg,
FedProx and FedAMW with independent clients.

``client_eval`` ('test', 'val' or 'both'; ``--client-eval``) scores every client's local model
each round (``stats['client_eval']``, functions/tools.py) and adds ``client_test_loss`` /
``client_test_acc`` (and the ``client_val_*`` pair) to the results: each a list with one entry
per algorithm in ``name``'s order -- a list over the repeats of [Round, N] arrays (DL and
FedAMW_OneShot: [N]), or None where the algorithm has no client models (CL), no validation set
('val' outside FedAMW and FedAMW_OneShot) or was skipped.  The reference's keys and shapes stay
untouched; without the option the keys are absent.

``local_eval`` ('global', 'own' or 'both'; ``--local-eval``) scores the round's global model
and / or every client's own model on each client's OWN training rows (``stats['local_eval']``)
and adds ``local_global_loss`` / ``local_global_acc`` / ``global_objective`` and the
``local_own_*`` pair in the same per-algorithm list form (``global_objective``: [Round]; DL:
[N] and a 0-dim objective; FedAMW_OneShot: 'own' [N]); None for CL, which pools the clients.
"""
import argparse
import os
import pickle
import time

import numpy as np
import torch

from .functions import tools, utils
from .functions.optimal_parameters import get_parameter
from . import engine

NAMES = ['CL', 'DL', 'FedAMW_OneShot', 'FedAvg', 'FedProx', 'FedAMW']
# exp.py:124 leaves its FedNova call commented out: it runs only when ``algos`` names it, and its
# rows are then appended after the six above (the default result layout is unchanged)
# Scaffold (not in the reference) likewise: its row comes after FedNova's
# the FedOpt server optimizers (not in the reference) after Scaffold's, in this order
EXTRA = ['FedNova', 'Scaffold', 'FedAvgM', 'FedAdagrad', 'FedAdam', 'FedYogi']
# q-FedAvg (not in the reference) after the FedOpt rows; a list of its own, so that EXTRA keeps its value
EXTRA_FAIR = ['QFedAvg']
# the robust aggregates (not in the reference) after q-FedAvg's row, in this order; again a list of its own
EXTRA_ROBUST = ['FedMedian', 'FedTrimmedMean']
# Krum and Multi-Krum (not in the reference) after the robust rows, in this order; once more a list of its own
EXTRA_KRUM = ['Krum', 'MultiKrum']
# RFA, the geometric median (not in the reference) after the Krum rows; a list of its own as well
EXTRA_RFA = ['FedRFA']
# FedTopK, top-k sparsified uploads with error feedback (not in the reference) after RFA's row; a list of its own too
EXTRA_TOPK = ['FedTopK']
# DPFedAvg, clipped updates and Gaussian noise (not in the reference) after FedTopK's row; a list of its own too
EXTRA_DP = ['DPFedAvg']


def prepare(dataset, D, num_partitions, alpha_Dirk, params, data_dir, synth=None, verbose=True):
    """exp.py:60-99 for one repeat.  Returns dict(X_train [list of N GPU tensors], y_train,
    X_test, y_test, X_val, y_val, validloader, heterogeneity, index_partitions)."""
    X, y, Xt, yt, parts, d, C = utils.load_full_data(dataset, num_partitions, alpha_Dirk, data_dir, synth=synth,
                                                     verbose=verbose)
    order = utils.full_batch_order(len(y), shuffle=True)                          # exp.py:61
    utils.full_batch_order(len(yt), shuffle=False)                                # exp.py:62
    X, y = X[order], torch.from_numpy(y[order]).long()
    yt = torch.from_numpy(yt).long()
    phi, phi_t = tools.feature_mapping(torch.from_numpy(X).reshape(1, X.shape[0], X.shape[1]), torch.from_numpy(Xt),
                                       params['kernel_par'], D, params['kernel_type'])
    phi = phi.reshape(-1, D)
    dev = phi.device
    Xc = [phi[torch.as_tensor(np.asarray(idx, dtype=np.int64), device=dev)] for idx in parts]
    yc = [y[np.asarray(idx, dtype=np.int64)] for idx in parts]
    hete, _ = engine.heterogeneity(engine.Features(Xc, yc, D, dev))               # exp.py:66-74
    Xv, yv, Xtr, ytr = [], [], [], []
    for Xi, yi in zip(Xc, yc):                                                    # exp.py:78-90
        ridx = np.arange(Xi.shape[0])
        np.random.shuffle(ridx)
        cut = int(Xi.shape[0] * 0.2)
        vi, ti = ridx[:cut], ridx[cut:]
        Xv.append(Xi[torch.from_numpy(vi).to(dev)])
        yv.append(yi[vi])
        Xtr.append(Xi[torch.from_numpy(ti).to(dev)])
        ytr.append(yi[ti])
    X_val, y_val = torch.cat(Xv, 0).cpu(), torch.cat(yv, 0)
    vl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X_val, y_val), batch_size=16, shuffle=True)
    return dict(X_train=Xtr, y_train=ytr, X_test=phi_t, y_test=yt, X_val=X_val, y_val=y_val, validloader=vl,
                heterogeneity=hete, index_partitions=parts, num_classes=C, d=d)


def run(dataset='a9a', D=2000, num_partitions=10, local_epoch=2, Round=100, batch_size=32, n_repeats=1,
        alpha_Dirk=0.01, data_dir='../FedAMW/datasets/', result_dir='./results', save=True, clients='sequential',
        algos=tuple(NAMES), synth=None, verbose=True, client_eval=None, local_eval=None, participation=None,
        sample_seed=0, server_lr=None, server_beta1=0.9, server_beta2=0.99, server_tau=1e-3, qffl_q=1.0,
        qffl_weighting='size', robust_trim=0.1, byzantine_fraction=0.0, byzantine_attack='sign_flip',
        byzantine_scale=1.0, krum_f=0.1, rfa_iters=3, rfa_nu=1e-6, rfa_init='start', rfa_weighting='size',
        topk_ratio=0.01, topk_memory=True, dp_clip=1.0, dp_noise_multiplier=1.0, dp_noise_seed=0,
        dp_weighting='uniform', dp_adaptive_quantile=None, dp_adaptive_lr=0.2):
    if client_eval not in (None, 'test', 'val', 'both'):
        raise ValueError("client_eval must be None, 'test', 'val' or 'both'")
    if local_eval not in (None, 'global', 'own', 'both'):
        raise ValueError("local_eval must be None, 'global', 'own' or 'both'")
    known = NAMES + EXTRA + EXTRA_FAIR + EXTRA_ROBUST + EXTRA_KRUM + EXTRA_RFA + EXTRA_TOPK + EXTRA_DP
    unknown = [n for n in algos if n not in known]
    if unknown:
        raise ValueError('unknown algorithm(s) %s (known: %s)' % (', '.join(unknown), ', '.join(known)))
    names = list(NAMES) + [n for n in EXTRA + EXTRA_FAIR + EXTRA_ROBUST + EXTRA_KRUM + EXTRA_RFA + EXTRA_TOPK
                           + EXTRA_DP if n in algos]
    lwant = {None: (), 'both': ('global', 'own')}.get(local_eval, (local_eval,))
    want = {None: (), 'both': ('test', 'val')}.get(client_eval, (client_eval,))
    cev = {'client_%s_%s' % (w, m): [None] * len(names) for w in want for m in ('loss', 'acc')}
    cev.update({'local_%s_%s' % (w, m): [None] * len(names) for w in lwant for m in ('loss', 'acc')})
    if 'global' in lwant:
        cev['global_objective'] = [None] * len(names)
    torch.manual_seed(100)
    np.random.seed(100)
    P = get_parameter(dataset)
    task, C, k_par = P['task_type'], P['num_classes'], P['kernel_par']
    lr, mu, lam = P['lr'], P['lambda_prox'], P['lambda_reg']
    lr_p, lr_p_os, lam_os = P.get('lr_p', 1e-3), P.get('lr_p_os', 1e-3), P.get('lambda_reg_os', P['lambda_reg'])
    train_mat = np.empty((len(names), Round, n_repeats))
    error_mat = np.empty((len(names), Round, n_repeats))
    acc_mat = np.empty((len(names), Round, n_repeats))
    hete_mat = np.empty(n_repeats)
    timing = {}
    # partial participation (FedAvg, FedProx and FedNova only, which then run with parallel clients):
    # participants[k][repeat] = the R sampled id arrays of algorithm k's call
    participants = [None] * len(names)

    def keep_participants(name, st):
        if participation is not None:
            k = names.index(name)
            participants[k] = (participants[k] or []) + [st['participants']]

    for t in range(n_repeats):
        d = prepare(dataset, D, num_partitions, alpha_Dirk, P, data_dir, synth=synth, verbose=verbose)
        C = d['num_classes'] if task == 'classification' else C
        hete_mat[t] = d['heterogeneity']
        a = (d['X_train'], d['y_train'], d['X_test'], d['y_test'])
        kw = dict(verbose=verbose)
        par = dict(clients=clients, **kw)
        fpar = par if participation is None else dict(clients='parallel', participation=participation,
                                                      sample_seed=sample_seed, **kw)

        def timed(name, fn):
            t0 = time.perf_counter()
            out = fn()
            timing.setdefault(name, []).append(time.perf_counter() - t0)
            return out

        def ce(name, has_val):
            """The ``stats`` dict of one algorithm call (None without --client-eval / --local-eval,
            or when all that was asked for is 'val' and the algorithm has no validation set)."""
            req = tuple(w for w in want if w == 'test' or has_val)
            st = {'client_eval': req} if req else {}
            if lwant:
                st['local_eval'] = lwant
            st = st or None
            if st is not None:
                calls.append((names.index(name), st))
            return st

        calls = []

        # exp.py:116-130, positional as the reference calls them; skipped algorithms leave NaN rows
        for k in range(len(names)):
            train_mat[k, :, t] = error_mat[k, :, t] = acc_mat[k, :, t] = np.nan
        if 'CL' in algos:
            r = timed('CL', lambda: tools.Centralized(*a, task, C, D, lr, local_epoch * Round, batch_size, False, 0,
                                                      False, 0, **kw))
            train_mat[0, :, t], error_mat[0, :, t], acc_mat[0, :, t] = float(r[0]), r[1], r[2]
        if 'DL' in algos:
            r = timed('DL', lambda: tools.Distributed(*a, task, C, D, lr, local_epoch * Round, batch_size, False, 0,
                                                      False, 0, stats=ce('DL', False), **kw))
            train_mat[1, :, t], error_mat[1, :, t], acc_mat[1, :, t] = float(r[0]), r[1], r[2]
        if 'FedAMW_OneShot' in algos:
            r = timed('FedAMW_OneShot', lambda: tools.FedAMW_OneShot(*a, d['validloader'], task, C, D, lr,
                                                                     local_epoch * Round, batch_size, False, 0, True,
                                                                     lam_os, Round, lr_p_os,
                                                                     stats=ce('FedAMW_OneShot', True), **kw))
            train_mat[2, :, t], error_mat[2, :, t], acc_mat[2, :, t] = float(r[0]), r[1].numpy(), r[2].numpy()
        if 'FedAvg' in algos:
            st = ce('FedAvg', False)
            if participation is not None:
                st = st or {}                  # always a stats dict: it carries the participants
            r = timed('FedAvg', lambda: tools.FedAvg(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False, 0,
                                                     Round, stats=st, **fpar))
            keep_participants('FedAvg', st)
            train_mat[3, :, t], error_mat[3, :, t], acc_mat[3, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        if 'FedProx' in algos:
            st = ce('FedProx', False)
            if participation is not None:
                st = st or {}                  # always a stats dict: it carries the participants
            r = timed('FedProx', lambda: tools.FedProx(*a, task, C, D, lr, local_epoch, batch_size, True, mu, False,
                                                       0, Round, stats=st, **fpar))
            keep_participants('FedProx', st)
            train_mat[4, :, t], error_mat[4, :, t], acc_mat[4, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        if 'FedAMW' in algos:
            r = timed('FedAMW', lambda: tools.FedAMW(*a, d['validloader'], task, C, D, lr, local_epoch, batch_size,
                                                     False, 0, True, lam, Round, lr_p, stats=ce('FedAMW', True),
                                                     **par))
            train_mat[5, :, t], error_mat[5, :, t], acc_mat[5, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        if 'FedNova' in algos:
            # exp.py:124's arguments; the reference form (tools.FedNova's variant='reference')
            st = ce('FedNova', False)
            if participation is not None:
                st = st or {}
            r = timed('FedNova', lambda: tools.FedNova(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False, 0,
                                                       Round, stats=st, **fpar))
            keep_participants('FedNova', st)
            train_mat[6, :, t], error_mat[6, :, t], acc_mat[6, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        if 'Scaffold' in algos:
            # FedAvg's arguments; clients are always parallel (classification only)
            st = ce('Scaffold', False)
            if participation is not None:
                st = st or {}
            spar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            r = timed('Scaffold', lambda: tools.Scaffold(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **spar))
            keep_participants('Scaffold', st)
            k = names.index('Scaffold')
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in ('FedAvgM', 'FedAdagrad', 'FedAdam', 'FedYogi'):
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel; server_lr None: the rule's default
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            opar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            opar.update(beta1=server_beta1, tau=server_tau)
            if server_lr is not None:
                opar['server_lr'] = server_lr
            if name == 'FedAvgM':
                del opar['tau']
            else:
                opar['beta2'] = server_beta2
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **opar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        if 'QFedAvg' in algos:
            # FedAvg's arguments; clients are always parallel
            st = ce('QFedAvg', False)
            if participation is not None:
                st = st or {}
            qpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            r = timed('QFedAvg', lambda: tools.QFedAvg(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False, 0,
                                                       Round, q=qffl_q, weighting=qffl_weighting, stats=st, **qpar))
            keep_participants('QFedAvg', st)
            k = names.index('QFedAvg')
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in EXTRA_ROBUST:
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel.  --byzantine-fraction > 0 corrupts that
            # share of the clients (ids fixed from seed 0) in both rows alike
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            rpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            if name == 'FedTrimmedMean':
                rpar['trim'] = robust_trim
            if byzantine_fraction > 0:
                rpar['byzantine'] = dict(fraction=byzantine_fraction, attack=byzantine_attack, scale=byzantine_scale)
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **rpar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in EXTRA_KRUM:
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel.  --krum-f for both rows, the --byzantine-*
            # flags as for the robust rows
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            kpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            kpar['f'] = krum_f
            if byzantine_fraction > 0:
                kpar['byzantine'] = dict(fraction=byzantine_fraction, attack=byzantine_attack, scale=byzantine_scale)
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **kpar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in EXTRA_RFA:
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel.  The --rfa-* flags, and the --byzantine-*
            # flags as for the robust and Krum rows
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            rpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            rpar.update(iters=rfa_iters, nu=rfa_nu, init=rfa_init, weighting=rfa_weighting)
            if byzantine_fraction > 0:
                rpar['byzantine'] = dict(fraction=byzantine_fraction, attack=byzantine_attack, scale=byzantine_scale)
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **rpar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in EXTRA_TOPK:
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel.  --topk-ratio and --topk-no-memory
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            tpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            tpar.update(ratio=topk_ratio, error_feedback=bool(topk_memory))
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **tpar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for name in EXTRA_DP:
            if name not in algos:
                continue
            # FedAvg's arguments; clients are always parallel.  The --dp-* flags, and the --byzantine-* flags
            st = ce(name, False)
            if participation is not None:
                st = st or {}
            dpar = dict(kw) if participation is None else dict(participation=participation, sample_seed=sample_seed,
                                                               **kw)
            dpar.update(clip=dp_clip, noise_multiplier=dp_noise_multiplier, noise_seed=dp_noise_seed,
                        weighting=dp_weighting)
            if dp_adaptive_quantile is not None:
                dpar['adaptive'] = dict(quantile=dp_adaptive_quantile, lr=dp_adaptive_lr)
            if byzantine_fraction > 0:
                dpar['byzantine'] = dict(fraction=byzantine_fraction, attack=byzantine_attack, scale=byzantine_scale)
            r = timed(name, lambda: getattr(tools, name)(*a, task, C, D, lr, local_epoch, batch_size, False, 0, False,
                                                         0, Round, stats=st, **dpar))
            keep_participants(name, st)
            k = names.index(name)
            train_mat[k, :, t], error_mat[k, :, t], acc_mat[k, :, t] = r[0].numpy(), r[1].numpy(), r[2].numpy()
        for k, st in calls:
            for key in cev:
                if key in st:
                    if cev[key][k] is None:
                        cev[key][k] = []
                    cev[key][k].append(st[key].numpy())
    data_ = {'epochs': Round, 'train_loss': train_mat, 'test_loss': error_mat, 'test_acc': acc_mat,
             'heterogeneity': hete_mat, 'name': names, 'seconds': {k: list(v) for k, v in timing.items()}}
    data_.update(cev)
    if participation is not None:
        data_['participants'] = participants
    if save:
        os.makedirs(result_dir, exist_ok=True)
        with open(os.path.join(result_dir, 'exp1_{}.pkl'.format(dataset)), 'wb') as f:
            pickle.dump(data_, f)
    return data_


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dataset', default='a9a')
    ap.add_argument('--D', type=int, default=2000)
    ap.add_argument('--clients', type=int, default=10, help='num_partitions')
    ap.add_argument('--local-epoch', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=100)
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--alpha', type=float, default=0.01, help='Dirichlet alpha (-1: uniform split)')
    ap.add_argument('--data-dir', default='../FedAMW/datasets/')
    ap.add_argument('--result-dir', default='./results')
    ap.add_argument('--mode', default='sequential', choices=['sequential', 'parallel'])
    ap.add_argument('--algos', default=','.join(NAMES),
                    help='comma-separated; FedNova (exp.py:124, commented out there), Scaffold, FedAvgM, FedAdagrad, '
                         'FedAdam, FedYogi, QFedAvg, FedMedian, FedTrimmedMean, Krum, MultiKrum, FedRFA, FedTopK and DPFedAvg run only when named here')
    ap.add_argument('--quiet', action='store_true')
    ap.add_argument('--client-eval', default=None, choices=['test', 'val', 'both'],
                    help="score every client's local model each round on the test / validation rows")
    ap.add_argument('--local-eval', default=None, choices=['global', 'own', 'both'],
                    help="score the round's global model / every client's own model on each client's own rows")
    ap.add_argument('--participation', type=float, default=None, metavar='F',
                    help='partial client participation: the fraction of the clients sampled per round, in (0, 1]. '
                         'Applies to the FedAvg, FedProx, FedNova, Scaffold, server-optimizer (FedAvgM, FedAdagrad, '
                         'FedAdam, FedYogi), QFedAvg, FedMedian, FedTrimmedMean, Krum, MultiKrum, FedRFA, FedTopK and DPFedAvg calls only, which then run with parallel clients '
                         'whatever --mode says; the other algorithms are unchanged')
    ap.add_argument('--sample-seed', type=int, default=0, metavar='S',
                    help='seed of the participation sampler (a private generator; with --participation)')
    ap.add_argument('--server-lr', type=float, default=None,
                    help='FedAvgM / FedAdagrad / FedAdam / FedYogi: the server learning rate (default: the rule\'s own)')
    ap.add_argument('--server-beta1', type=float, default=0.9, help='server momentum / first-moment decay')
    ap.add_argument('--server-beta2', type=float, default=0.99, help='second-moment decay (FedAdam, FedYogi)')
    ap.add_argument('--server-tau', type=float, default=1e-3, help='adaptivity of the adaptive server optimizers')
    ap.add_argument('--qffl-q', type=float, default=1.0, help='QFedAvg: the fairness exponent q >= 0 (0: FedAvg)')
    ap.add_argument('--qffl-weighting', default='size', choices=['size', 'uniform'],
                    help='QFedAvg: the client weights p_k, n_k / n or 1 / N')
    ap.add_argument('--robust-trim', type=float, default=0.1,
                    help='FedTrimmedMean: the fraction trimmed per side, in [0, 0.5)')
    ap.add_argument('--krum-f', type=float, default=0.1, metavar='F',
                    help='Krum, MultiKrum: the fraction of the clients that may misbehave, in [0, 0.5)')
    ap.add_argument('--rfa-iters', type=int, default=3, metavar='T',
                    help='FedRFA: the smoothed Weiszfeld iterations per round, in [0, 32]')
    ap.add_argument('--rfa-nu', type=float, default=1e-6, help='FedRFA: the smoothing nu > 0')
    ap.add_argument('--rfa-init', default='start', choices=['start', 'mean'],
                    help="FedRFA: iterate from the round-start model, or from the weighted mean as the paper does "
                         "(no robustness claim at few iterations)")
    ap.add_argument('--rfa-weighting', default='size', choices=['size', 'uniform'],
                    help='FedRFA: the client weights p_k, n_k / n or 1 / M')
    ap.add_argument('--topk-ratio', type=float, default=0.01, metavar='R',
                    help='FedTopK: the fraction of the C * D values every client uploads per round, in (0, 1]')
    ap.add_argument('--topk-no-memory', action='store_true',
                    help='FedTopK: drop what is not uploaded instead of keeping it in the client residual')
    ap.add_argument('--dp-clip', type=float, default=1.0, metavar='S',
                    help='DPFedAvg: the norm every client update is clipped to (inf: no clipping)')
    ap.add_argument('--dp-noise-multiplier', type=float, default=1.0, metavar='Z',
                    help='DPFedAvg: the noise multiplier z; the noise on the aggregate has standard deviation '
                         'z * S * max q (0: clipping only).  A simulator: no privacy accountant is provided')
    ap.add_argument('--dp-noise-seed', type=int, default=0, metavar='S', help='DPFedAvg: the seed of the device noise')
    ap.add_argument('--dp-weighting', default='uniform', choices=['size', 'uniform'],
                    help='DPFedAvg: the client weights q_k, 1 / M or n_k / n')
    ap.add_argument('--dp-adaptive-quantile', type=float, default=None, metavar='G',
                    help='DPFedAvg: adapt the clip to this quantile of the update norms (default: a fixed clip)')
    ap.add_argument('--dp-adaptive-lr', type=float, default=0.2, metavar='ETA',
                    help='DPFedAvg: the learning rate of the adaptive clip')
    ap.add_argument('--byzantine-fraction', type=float, default=0.0, metavar='F',
                    help='FedMedian, FedTrimmedMean, Krum, MultiKrum, FedRFA, DPFedAvg: the share of the clients that misbehave (0: none)')
    ap.add_argument('--byzantine-attack', default='sign_flip', choices=['sign_flip', 'gaussian', 'nan'],
                    help='what the misbehaving clients return')
    ap.add_argument('--byzantine-scale', type=float, default=1.0, help='the scale of sign_flip and gaussian')
    a = ap.parse_args(argv)
    out = run(a.dataset, a.D, a.clients, a.local_epoch, a.rounds, a.batch_size, a.repeats, a.alpha, a.data_dir,
              a.result_dir, True, a.mode, tuple(a.algos.split(',')), verbose=not a.quiet, client_eval=a.client_eval,
              local_eval=a.local_eval, participation=a.participation, sample_seed=a.sample_seed,
              server_lr=a.server_lr, server_beta1=a.server_beta1, server_beta2=a.server_beta2,
              server_tau=a.server_tau, qffl_q=a.qffl_q, qffl_weighting=a.qffl_weighting,
              robust_trim=a.robust_trim, byzantine_fraction=a.byzantine_fraction, byzantine_attack=a.byzantine_attack,
              byzantine_scale=a.byzantine_scale, krum_f=a.krum_f, rfa_iters=a.rfa_iters, rfa_nu=a.rfa_nu,
              rfa_init=a.rfa_init, rfa_weighting=a.rfa_weighting, topk_ratio=a.topk_ratio,
              topk_memory=not a.topk_no_memory, dp_clip=a.dp_clip, dp_noise_multiplier=a.dp_noise_multiplier,
              dp_noise_seed=a.dp_noise_seed, dp_weighting=a.dp_weighting,
              dp_adaptive_quantile=a.dp_adaptive_quantile, dp_adaptive_lr=a.dp_adaptive_lr)
    for k, name in enumerate(out['name']):
        print('%-15s final test acc %s' % (name, np.round(out['test_acc'][k, -1, :], 2)))
    print('heterogeneity', out['heterogeneity'], 'seconds', {k: np.round(v, 3) for k, v in out['seconds'].items()})
    return out
