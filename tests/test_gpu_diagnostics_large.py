"""The diagnostics kernels on draws whose element offsets pass 2**31 (byte offsets 2**34): a
[5 x 3 x 5] view at a draw stride of 2**29 + 3 elements inside a 17 GB buffer that is never
filled -- only the view's rows are written.  Every offset is formed in 64 bits; the results
equal the host restatement of the same 75 numbers bit for bit."""
import numpy as np
import pytest
import torch

import diagnostics_ref as DR
from binf_amd import diagnostics

pytestmark = pytest.mark.gpu

GIB = float(1 << 30)


def test_draw_stride_beyond_2_31_elements(device):
    free, _ = torch.cuda.mem_get_info(device)
    if free < 24 * GIB:
        pytest.skip('needs 24 GiB of free HBM, %.0f free' % (free / GIB))
    T, C, D = 5, 3, 5
    st, sc = (1 << 29) + 3, 7
    span = (T - 1) * st + (C - 1) * sc + D
    assert (T - 1) * st > 1 << 31
    x = DR.ar1(0.4, T, C, D, seed=77)
    whole = torch.empty(1 + span, dtype=torch.float64, device=device)
    view = s = mo = None
    try:
        view = whole[1:].as_strided((T, C, D), (st, sc, 1))
        view.copy_(torch.from_numpy(x))
        want = DR.diagnose(x, 2, 1)
        s = diagnostics.summary(view, max_lag=1)
        mo = diagnostics.chain_moments(view, split=2)
        for got, w in ((mo.mean, 'chain_mean'), (mo.m2, 'chain_m2'), (s.mean, 'post_mean'), (s.rhat, 'rhat'),
                       (s.ess, 'ess'), (s.mcse, 'mcse'), (s.truncated, 'truncated')):
            g = got.cpu().numpy()
            assert g.dtype == want[w].dtype and g.tobytes() == np.ascontiguousarray(want[w]).tobytes(), w
    finally:
        del whole, view, s, mo
        torch.cuda.empty_cache()
