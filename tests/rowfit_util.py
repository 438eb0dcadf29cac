"""How the GPU tests of the row-wise fits (test_gpu_als.py, test_gpu_lmf.py,
test_gpu_n2v.py) hand a table to a kernel: NaN in its padding columns and a
sentinel tail, both of which have to be as they were afterwards."""
import numpy as np
import torch

SENT = -123.0
PAD = 8            # sentinel values behind every output


def _padded(a, ld, tail=False):
    """float32 [n, f] as a flat device buffer of rows ld apart, NaN in the
    padding columns, PAD sentinels behind it if asked."""
    n, f = a.shape
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, :f] = a
    flat = buf.reshape(-1)
    if tail:
        flat = np.concatenate([flat, np.full(PAD, SENT, np.float32)])
    return torch.from_numpy(flat).cuda()


def _unpad(t, n, f, ld):
    """The live part of a padded buffer; asserts padding and tail."""
    h = t.cpu().numpy()
    assert (h[n * ld:] == SENT).all(), "values behind the table were written"
    m = h[:n * ld].reshape(n, ld)
    assert np.isnan(m[:, f:]).all(), "padding columns were written"
    return m[:, :f].copy()
