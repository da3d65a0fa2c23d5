"""bench.py --dump-outputs, without a GPU: which columns a dump keeps and that every dump stays within its 64 MB."""
import os

import numpy as np
import torch

import bench


def _bytes(B, L, N, rows, cols, with_field=True):
    return (2 * N + 3) * 8 * len(rows) + ((L * 2 * N + 1) * 8 * len(cols) if with_field else 0) + bench.DUMP_HEADER_BYTES


def test_dump_selection_stays_within_the_limit():
    for B, L, N in ((27, 200, 128), (216, 200, 128), (512, 200, 128), (3860, 200, 128), (4096, 200, 128), (8192, 200, 128),
                    (4096, 400, 256), (1, 800, 501), (10 ** 6, 200, 128), (10 ** 6, 4, 16)):
        for with_field in (True, False):
            rows, cols = bench.dump_selection(B, L, N, with_field)
            assert _bytes(B, L, N, rows, cols, with_field) <= bench.DUMP_LIMIT_BYTES, (B, L, N, with_field)
            assert len(rows) > 0 and np.all(np.diff(rows) > 0) and rows[-1] < B and np.all(np.isin(cols, rows))
            assert len(cols) > 0 if with_field else len(cols) == 0
            r2, c2 = bench.dump_selection(B, L, N, with_field)
            assert np.array_equal(rows, r2) and np.array_equal(cols, c2)               # fixed, not drawn afresh
    # every column whole when it fits; the rows of every column while they are a quarter of the limit at most
    rows, cols = bench.dump_selection(27, 200, 128)
    assert np.array_equal(rows, np.arange(27)) and np.array_equal(cols, rows)
    rows, cols = bench.dump_selection(4096, 200, 128)
    assert np.array_equal(rows, np.arange(4096)) and 0 < len(cols) < 136
    for B in (8192, 10 ** 6):
        rows, cols = bench.dump_selection(B, 200, 128)
        assert 0 < len(rows) < B and 0 < len(cols) < len(rows)


def test_dump_files_stay_within_the_limit(tmp_path):
    """The files themselves, at sizes where the rows of every column count (4096 columns) and where they are sampled too (8192,
    10^5 columns); the stand-in arrays repeat one column without allocating the batch."""
    for B, L, N in ((4096, 200, 128), (8192, 200, 128), (10 ** 5, 20, 64)):
        out = tmp_path / str(B)
        field = torch.arange(L * 2 * N, dtype=torch.float64).reshape(1, L, 2 * N).expand(B, L, 2 * N)
        n = torch.arange(B, dtype=torch.int32)
        files = bench.dump_outputs(str(out), L, N, field[:, 0, N:], field[:, L - 1, :N], n, torch.zeros(B, dtype=torch.int32), field,
                                   columns=np.arange(B) + 1000)
        assert files == sorted(os.listdir(out)) == ["I.npy", "I_columns.npy", "columns.npy", "n_orders.npy", "status.npy",
                                                    "surface_down.npy", "toa_up.npy"]
        assert sum(os.path.getsize(out / f) for f in files) <= bench.DUMP_LIMIT_BYTES
        d = {f[:-4]: np.load(out / f) for f in files}
        assert all(x.dtype == np.float64 for x in d.values())
        rows, cols = bench.dump_selection(B, L, N)
        assert np.array_equal(d["columns"], rows + 1000) and np.array_equal(d["I_columns"], cols + 1000)
        assert np.array_equal(d["n_orders"], rows) and d["toa_up"].shape == (len(rows), N) and d["I"].shape == (len(cols), L, 2 * N)
        assert np.array_equal(d["I"][0], field[0].numpy())
