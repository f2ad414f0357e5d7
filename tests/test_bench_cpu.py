"""CPU: the parts of bench.py that decide what a run computes and what --dump-outputs writes (no GPU needed)."""
import numpy as np

import bench


def test_synthetic_em_tiles_equal_the_serial_definition():
    """The threaded generator gives every tile the values of the serial loop over one generator (the benchmark's inputs stay
    the same from run to run and from build to build)."""
    from scipy.ndimage import gaussian_filter
    n, size, seed = 5, 24, 7
    rng = np.random.default_rng(seed)
    want = np.empty((n, size, size, size), np.uint8)
    for i in range(n):
        v = gaussian_filter(rng.random((size, size, size), dtype=np.float32), 2.0)
        v = (v - v.min()) / (v.max() - v.min())
        want[i] = (v * 255).astype(np.uint8)
    assert np.array_equal(bench.synthetic_em_tiles(n, size, seed), want)
    assert np.array_equal(bench.synthetic_em_tiles(n, size, seed), want)


def test_dump_outputs_whole_arrays_and_fixed_samples(tmp_path, monkeypatch):
    """Small arrays are written whole, large ones as the values at the same seeded positions on every call; always float32."""
    monkeypatch.setattr(bench, 'DUMP_MAX_VALUES', 1000)
    small = np.arange(600, dtype=np.uint8).reshape(2, 300)
    big = np.random.default_rng(1).integers(0, 256, (5, 40, 50), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / 'a'), {'small': small, 'big': big})
    bench.dump_outputs(str(tmp_path / 'b'), {'big': big})
    s = np.load(tmp_path / 'a' / 'small.npy')
    assert s.dtype == np.float32 and np.array_equal(s, small)
    b1, b2 = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'b' / 'big.npy')
    assert b1.dtype == np.float32 and b1.shape == (1000,) and np.array_equal(b1, b2)
    pos = np.sort(np.random.default_rng(0).integers(0, big.size, 1000))
    assert np.array_equal(b1, big.reshape(-1)[pos])
