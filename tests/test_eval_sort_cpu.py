"""The two debug calls of rl_eval_lists' length classes answer without a device, and refuse a null pointer or a short array."""
import ctypes as C

import numpy as np

from ranklib_amd import _native as N


def test_eval_classes_and_path_need_no_device_and_check_their_arguments():
    e = N.eval_classes()
    assert 0 < e["tiny"] < e["wave"] <= e["block"] < e["sort_lds"] and e["sort_lds"] * 12 <= 160 * 1024 and e["tile"] <= e["sort_lds"]
    assert sorted(N.eval_path()) == sorted(N.EVAL_CLASSES) and min(N.eval_path().values()) >= 0
    L, buf, n = N.lib(), np.zeros(8, np.int64), C.c_int32(0)
    for rc in (L.rl_debug_eval_classes(None, 5, C.byref(n)), L.rl_debug_eval_classes(buf.ctypes.data, 5, None),
               L.rl_debug_eval_classes(buf.ctypes.data, 4, C.byref(n)), L.rl_debug_eval_path(None, 5), L.rl_debug_eval_path(buf.ctypes.data, 4)):
        assert rc == -1 and b"rl_debug_eval_" in L.rl_last_error() and not buf.any()
