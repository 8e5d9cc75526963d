"""The trainer's host-side policies (nnnoiseless_amd/fit.py): plain Python, no library and no device."""
import numpy as np
import pytest

from nnnoiseless_amd import fit


def _rows(targets):
    """Rows [len(targets), 87] whose 22 targets are the given lists (padded with -1)."""
    rows = np.zeros((len(targets), 87), np.float32)
    rows[:, 42:64] = -1.0
    for i, t in enumerate(targets):
        rows[i, 42:42 + len(t)] = t
    return rows


def test_row_weights_classes_and_totals():
    """Three classes by the mean of the targets that are not -1; each class's weights add up to a third of the number of rows; a row
    with no target weighs 0."""
    rows = _rows([[0.1, 0.2], [0.9], [0.8, 1.0, 0.9], [0.5], [], [0.0, -1, 0.3], [0.34], [0.66], [0.7, 0.1]])
    w = fit.row_weights(rows)
    assert w.dtype == np.float32 and w.shape == (9,)
    lo, hi, med = [0, 5], [1, 2], [3, 6, 7, 8]          # [0.0, -1, 0.3] has mean 0.15, [0.7, 0.1] has mean 0.4
    for cls in (lo, hi, med):
        assert np.allclose(w[cls].sum(), 9 / 3) and np.allclose(w[cls], 3 / len(cls))
    assert w[4] == 0.0
    # the same through leading dimensions
    assert np.array_equal(fit.row_weights(rows.reshape(3, 3, 87)), w.reshape(3, 3))


def test_row_weights_empty_class():
    """The deliberate deviation: a class without a member contributes nothing (the reference divides by zero: every weight NaN)."""
    w = fit.row_weights(_rows([[0.1], [0.2], [0.9], []]))
    assert np.isfinite(w).all()
    assert np.allclose(w, [4 / 2 / 3, 4 / 2 / 3, 4 / 1 / 3, 0.0])
    assert not fit.row_weights(_rows([[], []])).any()


def test_windows():
    count, S, window = 11, 3, 4
    rows = np.arange(count * S * 87, dtype=np.float32).reshape(count, S, 87)
    seqs = fit.windows(rows, window)
    assert seqs.shape == (S * 2, window, 87)            # 11 // 4 = 2 windows per stream, 3 rows dropped
    for s in range(S):
        for k in range(2):
            assert np.array_equal(seqs[2 * s + k], rows[k * window:(k + 1) * window, s])
    assert fit.windows(rows, 12).shape == (0, 12, 87)
    with pytest.raises(ValueError):
        fit.windows(rows[..., :86], window)


def test_validation_split_is_the_last_fraction():
    assert fit.validation_split(10, 0.1) == (9, 1)
    assert fit.validation_split(75, 0.1) == (67, 8)     # int(75 * 0.9) = 67, as Keras splits
    assert fit.validation_split(5, 0.0) == (5, 0)


def test_batch_plan_short_last_batch():
    plan = fit.batch_plan(70, 32, np.random.default_rng(1))
    assert [len(b) for b in plan] == [32, 32, 6]
    assert sorted(np.concatenate(plan)) == list(range(70))
    again = fit.batch_plan(70, 32, np.random.default_rng(2))
    assert not np.array_equal(np.concatenate(plan), np.concatenate(again))


def test_fit_drives_the_trainer_by_the_plan():
    """fit on a stand-in trainer: which sequences each call sees, the layout it hands over, the held-out tail, the short batch."""
    class Stub:
        def __init__(self):
            self.grads, self.losses_, self.steps = [], [], 0

        def grad(self, rows, w):
            assert rows.shape[0] == 5 and rows.shape[2] == 87 and w.shape == rows.shape[:2] and rows.flags.c_contiguous
            self.grads.append(rows[0, :, 0].copy())
            return {"total": 2.0}

        def loss(self, rows, w):
            self.losses_.append(rows[0, :, 0].copy())
            return {"total": 4.0}

        def step(self):
            self.steps += 1

    count, S, window = 26, 3, 5                         # 5 windows per stream, 15 sequences: 13 train, 2 held out
    rows = np.zeros((count, S, 87), np.float32)
    rows[..., 0] = np.arange(count)[:, None] + 100 * np.arange(S)[None, :]   # feature 0 names (stream, row)
    rows[..., 42:64] = 0.5
    stub = Stub()
    h = fit.fit(stub, rows, epochs=2, batch=4, window=window, validation=0.1, seed=3)   # int(15 * 0.9) = 13
    first = np.array([100 * s + window * k for s in range(S) for k in range(5)], np.float32)   # each sequence's first row
    assert stub.steps == 2 * 4 and [len(g) for g in stub.grads] == [4, 4, 4, 1] * 2
    for e in range(2):
        assert sorted(np.concatenate(stub.grads[4 * e:4 * e + 4])) == sorted(first[:13])
    assert not np.array_equal(np.concatenate(stub.grads[:4]), np.concatenate(stub.grads[4:]))     # shuffled anew
    assert [list(l) for l in stub.losses_] == [list(first[13:])] * 2
    assert h == {"loss": [2.0, 2.0], "val_loss": [4.0, 4.0]}
    assert fit.fit(Stub(), rows, epochs=1, batch=4, window=window, validation=0.0)["val_loss"] == [None]
    with pytest.raises(ValueError):
        fit.fit(Stub(), rows, window=27)


def test_glorot_params_bounds():
    p = fit.glorot_params(np.random.default_rng(0))
    assert p.dtype == np.float32 and p.shape == (fit.PARAMS,)
    for name, (off, shape) in fit.TENSORS.items():
        v = p[off:off + int(np.prod(shape))]
        if len(shape) == 1:
            assert not v.any(), name
        else:
            limit = min(np.sqrt(6.0 / sum(shape)), fit.CLIP)
            assert np.abs(v).max() <= np.float32(limit) and np.abs(v).max() > 0.8 * limit, name
            if v.size > 1000:
                assert abs(v.mean()) < 0.05 * limit and 0.5 * limit < v.std() < 0.65 * limit, name   # uniform: limit / sqrt(3)
    # (the widest limit, the 24 -> 1 layer's sqrt(6 / 25) = 0.49, is just inside the reference's clip; a tighter clip caps)
    capped = fit.glorot_params(np.random.default_rng(0), clip=0.1)
    assert np.abs(capped).max() == np.float32(0.1) and (np.abs(capped[87478:87502]) == np.float32(0.1)).sum() > 12
    assert not np.array_equal(p, fit.glorot_params(np.random.default_rng(1)))
