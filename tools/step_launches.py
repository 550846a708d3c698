#!/usr/bin/env python3
"""The kernel launches of whole training steps, for comparing two builds of the library launch by launch and bit by bit.

  rocprofv3 --kernel-trace --stats -d DIR -o NAME -f csv -- python tools/step_launches.py run
      ResNet-50 at batch 8 on synthetic batches, per configuration two steps with the running statistics tracked and one eval pass
      behind them: fp32 and bf16 under FAST and RECOMPUTE_BN, fp32 under FULL (whose eval pass the library refuses: none is run),
      fp32 FAST under the weight-gradient overlap modes 0, 1 and 2.  Each configuration ends in one line with a SHA-256 over every
      parameter tensor, the running statistics and the eval pass's pred: two builds that compute the same print the same lines.
      RESNET_MI_LIB selects the build
  python tools/step_launches.py compare A_kernel_trace.csv B_kernel_trace.csv
      the ordered lists of (kernel name, grid, workgroup) of two such traces, in dispatch order; exit status 1 where they differ
"""
import csv
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def configurations(B):
    f32, bf16 = B.MI_DTYPE_F32, B.MI_DTYPE_BF16
    fast, rc, full = B.MI_STORE_FAST, B.MI_STORE_RECOMPUTE_BN, B.MI_STORE_FULL
    return ([("f32 FAST", f32, fast, None), ("f32 RECOMPUTE_BN", f32, rc, None), ("bf16 FAST", bf16, fast, None),
             ("bf16 RECOMPUTE_BN", bf16, rc, None), ("f32 FULL", f32, full, None)] +
            [("f32 FAST overlap %d" % m, f32, fast, m) for m in (0, 1, 2)])


def run():
    sys.path.insert(0, ROOT)
    from resnet_amd import Trainer, resnet_dims, binding as B
    for name, dtype, policy, overlap in configurations(B):
        tr = Trainer(resnet_dims(), 8)
        tr.set_store_policy(policy)
        tr.set_dtype(dtype)
        if overlap is not None:
            tr.L.mi_trainer_set_overlap(tr.t, overlap)
        tr.source_synthetic()
        tr.track_running_stats(0.1)
        for _ in range(2):
            tr.load_new_batch()
            tr.forward()
            tr.backward()
            tr.update()
        tr.check()
        loss = tr.loss()[0]
        h = hashlib.sha256()
        for i in range(tr.n_locations):
            h.update(tr.get("params", i).tobytes())
        for a in tr.running_stats():
            h.update(a.tobytes())
        if policy != B.MI_STORE_FULL:
            tr.load_new_batch()
            tr.eval_forward()
            tr.check()
            h.update(tr.activation("softmax").tobytes())
        print("%s: loss of the second step %.6f, sha256 %s" % (name, loss, h.hexdigest()))
        tr.close()


def launches(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y",
                                                           "Workgroup_Size_Z")) for r in rows]


def compare(a, b):
    la, lb = launches(a), launches(b)
    print("%s: %d launches, %s: %d launches" % (a, len(la), b, len(lb)))
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print("first difference at launch %d:\n  %s\n  %s" % (i, x, y))
            return 1
    if len(la) != len(lb):
        print("one trace is a prefix of the other")
        return 1
    print("the same launches in the same order")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
