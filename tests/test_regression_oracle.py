"""models/regression.py train_one, the host PA regression rule (the Python CPU
server's training step and the oracle of the GPU regression tests): an index
repeated inside a sample counts once per occurrence."""
import numpy as np

from jubatus_amd.models.regression import train_one


def test_train_one_repeated_index_takes_every_increment():
    w = np.array([0.5, -1.0, 2.0, 0.0], np.float32)
    stats = np.zeros(3)
    idx, val = [2, 0, -1, 2, 2], [0.5, 1.0, 9.0, -0.25, 1.5]
    # w.x and ||x||^2 per occurrence, the -1 slot skipped
    dot = 0.5 * 2.0 + 1.0 * 0.5 - 0.25 * 2.0 + 1.5 * 2.0
    nrm = 0.25 + 1.0 + 0.0625 + 2.25
    y = dot + 1.0                                   # err = 1, the first sample: stddev 0, loss = 1
    train_one(w, stats, idx, val, y, 0.5, 0.1)      # C = 0.5 clips
    c = 0.5 / nrm
    want = [0.5 + c * 1.0, -1.0, 2.0 + c * (0.5 - 0.25 + 1.5), 0.0]
    np.testing.assert_allclose(w, want, rtol=1e-6)
    np.testing.assert_allclose(stats, [y, y * y, 1.0])


def test_train_one_degenerate_samples_change_statistics_only():
    w = np.array([0.5, -1.0], np.float32)
    stats = np.zeros(3)
    for idx, val in (([], []), ([-1, -1], [1.0, 2.0]), ([0, 1], [0.0, 0.0])):
        train_one(w, stats, idx, val, 3.0, 1.0, 0.1)
    np.testing.assert_array_equal(w, np.array([0.5, -1.0], np.float32))
    np.testing.assert_allclose(stats, [9.0, 27.0, 3.0])
