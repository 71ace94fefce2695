"""ofdg_set_front_batches is declared in include/ofdg.h, exported by libofdg.so and bound as Generator.set_front_batches
(no GPU needed; what it does is in test_gpu_paired_front.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_front_batches_is_declared_exported_and_bound(ofdg):
    header = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    assert re.search(r"^int ofdg_set_front_batches\(ofdg_ctx\* ctx, int n\);", header, re.M)
    assert "ofdg_set_front_batches" in ofdg.EXPORTS
    fn = ofdg.lib().ofdg_set_front_batches
    assert [a.__name__ for a in fn.argtypes] == ["c_void_p", "c_int"]
    assert callable(ofdg.Generator.set_front_batches)
    # a null context is refused without touching a device
    assert fn(None, 2) == ofdg.EINVAL
