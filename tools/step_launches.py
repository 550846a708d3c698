#!/usr/bin/env python3
"""The kernel launches of whole training steps, for comparing two builds of the library launch by launch.

  rocprofv3 --kernel-trace --stats -d DIR -o NAME -f csv -- python tools/step_launches.py run
      two steps of ResNet-50 at batch 8 in fp32, then two in bf16 (synthetic batches); RESNET_MI_LIB selects the build
  python tools/step_launches.py compare A_kernel_trace.csv B_kernel_trace.csv
      the ordered lists of (kernel name, grid, workgroup) of two such traces, in dispatch order; exit status 1 where they differ
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path.insert(0, ROOT)
    from resnet_amd import Trainer, resnet_dims, binding as B
    for dtype in (B.MI_DTYPE_F32, B.MI_DTYPE_BF16):
        tr = Trainer(resnet_dims(), 8)
        tr.set_dtype(dtype)
        tr.source_synthetic()
        for _ in range(2):
            tr.load_new_batch()
            tr.forward()
            tr.backward()
            tr.update()
        tr.check()
        print("dtype %d: loss of the second step %.6f" % (dtype, tr.loss()[0]))
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
