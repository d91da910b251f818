"""Golden vectors for partial client participation (``part_*.npz``).

Run only where the reference is installed: ``python tests/golden/make_golden_participation.py``.
It imports the reference through ``make_golden`` (``T``, unmodified) and reuses its ``synth`` and
``_split``; nothing else in the repository imports the reference.

The harness is ``make_golden._fed_par`` restricted to a round's sampled clients: every sampled
client trains a fresh ``copy.deepcopy`` of the round's global model with the reference's own
``train_loop`` (so only the sampled clients' DataLoader passes draw from the global generator, in
ascending client id), the weights are ``n[S] / sum(n[S])`` (tools.py:333 restricted to S), the
train loss and the aggregate are tools.py:344-349 over S in ascending client id, then the
reference's ``test_loop``.  The schedule is ``sorted(torch.randperm(N, generator=g)[:M])`` per
round on a private generator seeded with ``sample_seed``.

Each file holds the usual keys (inputs, hyper-parameters, the three returns, ``W`` after every
round) plus ``sched`` [R][M], ``sample_seed``, ``M`` and ``rng_after`` (four draws from the global
generator after the run: where the run left it).
"""
import contextlib
import copy
import io
import os

import numpy as np
import torch

import make_golden as MG

T = MG.T
OUT = os.path.dirname(os.path.abspath(__file__))
TORCH_SEED = 100


def schedule(N, M, R, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return [np.sort(torch.randperm(N, generator=g)[:M].numpy()) for _ in range(R)]


def _fed_part(X_train, y_train, X_test, y_test, type, num_classes, D, lr, epoch, batch_size, prox, mu,
              lambda_reg_if, lambda_reg, round, sched):
    """FedAvg / FedProx over the sampled clients of each round, parallel clients."""
    model = T.MLP(D, num_classes).to(T.device)
    n = np.array([len(y) for y in y_train])
    out = [torch.zeros(round) for _ in range(3)]
    for t in range(round):
        lr = T.update_learning_rate(t, lr, round)
        S = sched[t]
        p = torch.tensor(n[S] / sum(n[S]), dtype=torch.float32)
        Ws, losses = [], []
        for i in S:
            local = copy.deepcopy(model)
            w, l, _ = T.train_loop(X_train[i], y_train[i], type=type, model=local, lr=lr, epoch=epoch,
                                   batch_size=batch_size, prox=prox, mu=mu, lambda_reg_if=lambda_reg_if,
                                   lambda_reg=lambda_reg)
            Ws.append(copy.deepcopy(w)['classifier.weight'])
            losses.append(l)
        out[0][t] = torch.sum(p * torch.tensor(losses))
        g = Ws[0] * p[0]
        for j in range(1, len(Ws)):
            g = g + p[j] * Ws[j]
        model.load_state_dict({'classifier.weight': g})
        out[1][t], out[2][t] = T.test_loop(X_test=X_test, y_test=y_test, type=type, model=model,
                                           batch_size=batch_size)
    return out


CASES = [
    # name, algo, data kwargs, hyper-parameters, M, sample_seed
    ('part_fedavg', 'fedavg', dict(seed=21, sizes=[45, 32, 7, 64, 20, 33], n_test=50, n_raw=12, D=64, C=4),
     dict(lr=0.5, epoch=2, batch_size=32, prox=False, mu=0.0, reg=False, lam=0.0, R=4), 3, 7),
    ('part_fedprox_reg', 'fedprox', dict(seed=22, sizes=[33, 65, 1, 20, 96, 40, 12], n_test=61, n_raw=10, D=128, C=7),
     dict(lr=0.5, epoch=2, batch_size=32, prox=True, mu=0.05, reg=True, lam=0.001, R=4), 2, 8),
    # B = 100 > 64: the batch-tiled (wide) training form
    ('part_fedavg_one', 'fedavg', dict(seed=23, sizes=[40, 25, 70, 9, 31], n_test=47, n_raw=14, D=96, C=10),
     dict(lr=0.3, epoch=1, batch_size=100, prox=False, mu=0.0, reg=False, lam=0.0, R=5), 1, 9),
]


def run_case(name, algo, dk, hp, M, sample_seed):
    d = MG.synth(**dk)
    Xs, ys, Xt, yt = MG._split(d)
    C, D = dk['C'], dk['D']
    sched = schedule(len(Xs), M, hp['R'], sample_seed)
    MG._trace['W'].clear()
    MG._trace['p'].clear()
    torch.manual_seed(TORCH_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        tr, tl, ta = _fed_part(Xs, ys, Xt, yt, 'classification', C, D, hp['lr'], hp['epoch'], hp['batch_size'],
                               hp['prox'], hp['mu'], hp['reg'], hp['lam'], hp['R'], sched)
    rng_after = torch.empty(4, dtype=torch.int64).random_().numpy()
    rec = dict(d)
    rec.update({k: np.asarray(v) for k, v in hp.items()})
    rec.update(algo=algo, mode='par', C=C, D=D, torch_seed=TORCH_SEED, train_loss=tr.detach().numpy(),
               test_loss=tl.numpy(), test_acc=ta.numpy(), W=np.stack(MG._trace['W']),
               sched=np.stack(sched).astype(np.int64), sample_seed=sample_seed, M=M, rng_after=rng_after)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **rec)
    print(name, [s.tolist() for s in sched], 'acc', np.round(ta.numpy(), 2), 'loss', np.round(tr.detach().numpy(), 4))


if __name__ == '__main__':
    for case in CASES:
        run_case(*case)
