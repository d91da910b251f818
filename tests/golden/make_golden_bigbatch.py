"""Golden-vector generator for batch sizes above 64: runs the UNMODIFIED reference
``functions/tools.py`` (imported through make_golden.py, as make_golden_mse.py does) at
``batch_size`` 65, 100, 256 and full batch.

Run only in the build container: ``python tests/golden/make_golden_bigbatch.py``.  Writes data
only, every file named ``bb_*`` (tests/fixtures.py globs ``fed*``, ``unit_train_*``,
``long_fed*``, ``bench_fedamw_*``, ``horizon_*``: none may match), each under 300 KB:

  bb_data.npz      the shared inputs, stored once (make_golden.synth, seed 41: raw width 12,
                   D = 80 so ld = 128 pads, C = 5): ragged clients of 130, 64, 257, 101 and 1
                   rows -- above and below the batch of 100, an exact 64-row block, tails of 1,
                   30 and 57 rows -- 50 test rows, 137 validation rows (Bv = 16: a ragged 9)
  bb_unit_<B>_<p>.npz  one train_loop call on client 2 (257 rows) from a start moved off the
                   initialisation, E = 3: B = 65 (tail 62), 100 (tail 57), 256 (tail 1) and
                   300 (full batch, B >= n); p = plain | proxridge
  bb_fedavg_seq, bb_fedavg_par, bb_fedprox_seq, bb_fedamw_par
                   R = 3 rounds at batch_size = 100, E = 2 (``par``: make_golden.py's harness
                   variant, a fresh copy of the global model per client; FedAMW with the
                   validation loader at batch 16)
  bb_central_256   Centralized at batch_size = 256 (553 pooled rows: 256, 256, 41), 3 epochs

Every case records ``rng_after``, the global generator's position after the call.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (imports the reference unmodified and wraps its test_loop)

T = G.T
_trace = G._trace
DATA = dict(seed=41, sizes=[162, 80, 321, 126, 1], n_test=50, n_raw=12, D=80, C=5, val_frac=0.2)
SIZES = [130, 64, 257, 101, 1]            # what val_frac leaves of DATA['sizes']
TORCH_SEED = 100
BV = 16
UNIT_CLIENT, UNIT_EPOCH = 2, 3
UNIT_B = (65, 100, 256, 300)
UNIT_TERMS = (('plain', False, False), ('proxridge', True, True))
ROUND_CASES = [
    ('bb_fedavg_seq', 'fedavg', 'seq', dict(lr=0.5, prox=False, mu=0.0, reg=False, lam=0.0)),
    ('bb_fedavg_par', 'fedavg', 'par', dict(lr=0.5, prox=False, mu=0.0, reg=False, lam=0.0)),
    ('bb_fedprox_seq', 'fedprox', 'seq', dict(lr=0.5, prox=True, mu=0.05, reg=True, lam=0.001)),
    ('bb_fedamw_par', 'fedamw', 'par', dict(lr=0.5, prox=False, mu=0.0, reg=True, lam=1e-4, lr_p=0.05)),
]
EPOCH, B, R = 2, 100, 3


def _f(v):
    return np.asarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)


def _rng_after():
    return torch.empty(4, dtype=torch.int64).random_().numpy()


def _valid(d):
    return torch.utils.data.DataLoader(
        torch.utils.data.TensorDataset(torch.from_numpy(d['X_val']), torch.from_numpy(d['y_val'])),
        batch_size=BV, shuffle=True)


def main():
    torch.set_num_threads(1)
    d = G.synth(**DATA)
    assert list(d['sizes']) == SIZES, d['sizes']
    C, D = DATA['C'], DATA['D']
    np.savez_compressed(os.path.join(HERE, 'bb_data.npz'), **d, torch_seed=TORCH_SEED, C=C, D=D, Bv=BV)
    Xs, ys, Xt, yt = G._split(d)
    for name, algo, mode, hp in ROUND_CASES:
        _trace['W'].clear()
        _trace['p'].clear()
        pos = ('classification', C, D, hp['lr'], EPOCH, B, hp['prox'], hp['mu'], hp['reg'], hp['lam'], R)
        torch.manual_seed(TORCH_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            if algo == 'fedamw':
                tr, tl, ta = {'seq': T.FedAMW, 'par': G._fedamw_par}[mode](Xs, ys, Xt, yt, _valid(d), *pos, hp['lr_p'])
            else:
                fn = {'seq': T.FedAvg if algo == 'fedavg' else T.FedProx, 'par': G._fed_par}[mode]
                tr, tl, ta = fn(Xs, ys, Xt, yt, *pos)
        rec = {k: np.asarray(v) for k, v in hp.items()}
        rec.update(algo=algo, mode=mode, epoch=EPOCH, batch_size=B, R=R, train_loss=_f(tr), test_loss=_f(tl),
                   test_acc=_f(ta), W=np.stack(_trace['W']), rng_after=_rng_after())
        if _trace['p']:
            rec['p'] = np.stack(_trace['p'])
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **rec)
        print(name, 'acc', np.round(_f(ta), 2), 'loss', np.round(_f(tr), 4))
    # Centralized at 256
    hp = dict(lr=0.5, epoch=3, prox=False, mu=0.0, reg=True, lam=0.001)
    _trace['W'].clear()
    _trace['p'].clear()
    torch.manual_seed(TORCH_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        tr, tl, ta = T.Centralized(Xs, ys, Xt, yt, 'classification', C, D, hp['lr'], hp['epoch'], 256, hp['prox'],
                                   hp['mu'], hp['reg'], hp['lam'])
    rec = {k: np.asarray(v) for k, v in hp.items()}
    rec.update(algo='centralized', batch_size=256, train_loss=_f(tr), test_loss=_f(tl), test_acc=_f(ta),
               W=np.stack(_trace['W']), rng_after=_rng_after())
    np.savez_compressed(os.path.join(HERE, 'bb_central_256.npz'), **rec)
    print('bb_central_256', 'acc', _f(ta), 'loss', _f(tr))
    # one train_loop call per (B, terms)
    X1, y1 = Xs[UNIT_CLIENT], ys[UNIT_CLIENT]
    for Bu in UNIT_B:
        for tag, prox, reg in UNIT_TERMS:
            torch.manual_seed(123)
            model = T.MLP(D, C)
            with torch.no_grad():
                model.classifier.weight.add_(0.05 * torch.randn(C, D))
            W0 = model.classifier.weight.detach().clone().numpy()
            torch.manual_seed(7)
            w, loss, _ = T.train_loop(X1, y1, 'classification', model, 0.7, UNIT_EPOCH, Bu, prox, 0.05, reg, 0.003)
            np.savez_compressed(os.path.join(HERE, 'bb_unit_%d_%s.npz' % (Bu, tag)), W0=W0,
                                W=w['classifier.weight'].numpy().copy(), loss=np.float64(loss), lr=0.7,
                                epoch=UNIT_EPOCH, batch_size=Bu, prox=prox, mu=0.05, reg=reg, lam=0.003, seed=7,
                                client=UNIT_CLIENT, rng_after=_rng_after())
            print('bb_unit_%d_%s' % (Bu, tag), 'loss', loss)


if __name__ == '__main__':
    main()
