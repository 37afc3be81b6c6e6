"""The step plan's host-side tables for a set of shapes, as int64 arrays: workspace layout, the twenty parameter
descriptors and the rider range in every option state.  rv_plan_create / bind / set_option / descs / riders / buffer touch
no device, so this runs on fake base addresses, without a GPU.

    python tools/plan_tables.py            # rewrite tests/golden/plan_tables.npz from the library as built

tests/test_host_cpu.py::test_plan_tables_match_the_recorded_layout compares `tables()` of the current library with that
file, which was recorded from the commit before csrc/plan.hip got typed workspace ids and one derivation of d_flat.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "plan_tables.npz")

SHAPES = [(32, 64, 96, 8), (2137, 1000, 96, 100), (1024, 1024, 2048, 64), (4096, 1024, 2048, 64), (8192, 1024, 2048, 128),
          (4096, 1024, 2048, 256), (131072, 1024, 2048, 256)]
# every buffer of the workspace, in layout order (the list in the header comment of rv_plan_buffer)
NAMES = ["xb", "W1b", "Whb", "W3b", "W4b", "b1p", "bhp", "b3p", "b4p", "h1", "mulv_slabs", "mulv", "eps", "z", "h3", "dP4",
         "dP3", "dz_slabs", "dmulv", "dP1", "dW1", "dWh", "dWh_us", "dW3", "dW4", "dW1_us", "dW4_us", "db1p", "dbhp", "db3p",
         "db4p", "xq", "W1q", "W4q", "h3q", "dP4q", "dP1q", "fp8_state", "h3_amax", "ddp_flags", "mse_part", "kl_part"]
TENSORS = ["fc1.weight", "fc1.bias", "fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias", "fc3.weight", "fc3.bias",
           "fc4.weight", "fc4.bias"]
# fake, fixed, far apart: nothing is dereferenced
PARAM, EXP_AVG, EXP_AVG_SQ, GRAD, WORKSPACE, COUNTER, RING = (0x100000000, 0x200000000, 0x300000000, 0x400000000,
                                                              0x10000000000, 0x500000000, 0x500001000)


def _states(_lib):
    """(label, [(option, value), ...]) per recorded state: every combination of the three options that edit descriptors,
    each on a fresh plan, then the stages of two round trips on one plan each."""
    fp8, dt, fused = _lib.OPT_FP8, _lib.OPT_SLAB_DTYPE, _lib.OPT_LATENT_FUSED
    out = []
    for f8, half, fu in itertools.product((0, 1, 2), (_lib.SLAB_F32, _lib.SLAB_F16), (0, 1)):
        out.append(("fp8=%d slab=%s fused=%d" % (f8, "f16" if half == _lib.SLAB_F16 else "f32", fu),
                    [(fp8, f8), (dt, half), (fused, fu)]))
    out.append(("fused trip: as bound", []))
    out.append(("fused trip: 1->0", [(fused, 0)]))
    out.append(("fused trip: 1->0->1", [(fused, 0), (fused, 1)]))
    out.append(("fp8 trip: as bound", []))
    out.append(("fp8 trip: 0->1", [(fp8, 1)]))
    out.append(("fp8 trip: 0->1->0", [(fp8, 1), (fp8, 0)]))
    return out


def state_labels():
    from rawaudiovae_kelsey_amd import _lib
    return [s[0] for s in _states(_lib)]


def desc_fields():
    from rawaudiovae_kelsey_amd import _lib
    return [f[0] for f in _lib.ParamDesc._fields_]


def key(shape, what):
    return "%s_%d_%d_%d_%d" % ((what,) + tuple(shape))


def tables():
    """{key: int64 array} for every shape of SHAPES:
      ws_*      [2 + 2 * len(NAMES)]: rv_plan_workspace_bytes, (pointer - workspace, bytes) per name, then 1 if an unknown
                name gave NULL
      descs_*   [grad arena: without, with][state][from_flat 0, 1][tensor][field of rv_param_desc] (pointers as integers)
      riders_*  [grad arena: without, with][state][first, last]"""
    from rawaudiovae_kelsey_amd import _lib
    L = _lib.lib()
    states, fields = _states(_lib), desc_fields()
    out = {}
    for shape in SHAPES:
        descs = np.zeros((2, len(states), 2, 10, len(fields)), np.int64)
        riders = np.zeros((2, len(states), 2), np.int64)
        for with_grad in (0, 1):
            for si, (_, opts) in enumerate(states):
                plan = C.c_void_p()
                L.rv_plan_create(C.byref(plan), *shape)
                bufs = _lib.PlanBuffers(param=PARAM, exp_avg=EXP_AVG, exp_avg_sq=EXP_AVG_SQ, grad=GRAD if with_grad else None,
                                        workspace=WORKSPACE, step_counter=COUNTER, loss_ring=RING, ring=4)
                L.rv_plan_bind(plan, C.byref(bufs))
                for opt, value in opts:
                    L.rv_plan_set_option(plan, opt, value)
                arr = (_lib.ParamDesc * 10)()
                for from_flat in (0, 1):
                    L.rv_plan_descs(plan, arr, from_flat)
                    for t in range(10):
                        for fi, f in enumerate(fields):
                            descs[with_grad, si, from_flat, t, fi] = getattr(arr[t], f) or 0
                first, last = C.c_int(-1), C.c_int(-1)
                L.rv_plan_riders(plan, C.byref(first), C.byref(last))
                riders[with_grad, si] = first.value, last.value
                if with_grad == 0 and si == 0:
                    ws = [L.rv_plan_workspace_bytes(plan)]
                    for name in NAMES:
                        n = C.c_long(-1)
                        ptr = L.rv_plan_buffer(plan, name.encode(), C.byref(n))
                        ws += [(ptr or 0) - WORKSPACE, n.value]
                    ws.append(int(L.rv_plan_buffer(plan, b"no_such_buffer", None) is None))
                    out[key(shape, "ws")] = np.array(ws, np.int64)
                L.rv_plan_destroy(plan)
        out[key(shape, "descs")] = descs
        out[key(shape, "riders")] = riders
    return out


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    t = tables()
    np.savez_compressed(FIXTURE, **t)
    print("%s: %d arrays, %d bytes" % (FIXTURE, len(t), os.path.getsize(FIXTURE)))
