"""The single table of the library's RESNET_MI_* switches (README, "Environment switches").

Every switch is read once per process and selects another kernel instantiation, staging form, tile height or schedule.  ROUTES holds one
entry per (switch, value) with the operator cases that reach the code only that value reaches, the trainer configuration to re-run whole
steps in, the expected relation to the default route, and the launch names (mi_debug_trace_names: the names carry the instantiation's
parameters) the cases must produce.  EXEMPT lists the switches that select no kernel or are pinned elsewhere.  test_gpu_routes.py runs the
table, one child process per entry (tests/route_worker.py); test_route_table_names_every_switch holds it against the code and the README.

relation
  "bitwise"  the switch changes only staging, buffering, the vector width of an element-wise pass or the schedule: every output element
             sees the same sequence of fp32 operations, so outputs are compared bit for bit with the default child's
  "bounds"   the order of summation (tile height, k-split, reduction tree, which kernel) differs: the per-element bounds of perelement.py
Either way every case runs through its perelement.py checker against the float64 reference.

Operator cases: (checker, case, N) with the case tuples of perelement.py.  Shapes are (C, H, K, k, stride, N), picked with mi_conv_plan on
the host: small, and such that the plan or the variant differs from the default's; each list has a ragged last column tile (N * P no
multiple of 128) and whole tiles where the switch's precondition allows both.
"""
BF, F32 = "bf16", "f32"


def conv(dt, op, shape, route="default", where=""):
    C, H, K, k, s, N = shape
    return ("conv", (dt, route, op, C, H, K, k, s, where), N)


def convs(dt, ops, shapes, route="default"):
    return [conv(dt, op, sh, route) for sh in shapes for op in ops]


def conv_bn(dt, shape, route="default"):
    C, H, K, k, s, N = shape
    return ("conv_bn", ((dt, C, H, K, k, s, ""), route), N)


def dgrad_bn(dt, shape, where=""):
    C, H, K, k, s, N = shape
    return ("dgrad_bn", (dt, C, H, K, k, s, where), N)


# 64-pixel planes: columns N * 64 -- N = 5 ends in half a tile, N = 4 fills two
S_3x3 = (128, 8, 128, 3, 1, 5)
S_1x1 = (256, 8, 128, 1, 1, 5)
S_3x3s2 = (128, 8, 256, 3, 2, 5)
S_1x1_whole = (64, 8, 256, 1, 1, 4)
S_49 = (512, 7, 512, 3, 1, 3)            # planes of 49 pixels: the forms for P % 4 != 0
FD = ("fwd", "dgrad")
ALL = ("fwd", "dgrad", "wgrad")
# the direct VALU kernels (RESNET_MI_IGEMM=0): 448 pixels per workgroup
D_SHAPES = [(64, 8, 64, 3, 1, 4), (128, 8, 128, 3, 2, 4), (32, 8, 64, 3, 1, 4)]
D_CASES = convs(F32, FD, D_SHAPES) + [conv(F32, "fwd", (3, 32, 64, 7, 2, 4))]
DIRECT = {"RESNET_MI_IGEMM": "0"}
# BN over 7 x 7 planes (ResNet-50's last stage, trainer_bn_*_cases, at N = 3): 49 pixels hold a vector but are no multiple of one
BN7_FWD = [("bn_fwd", c, 3) for c in (("f32", 512, 7, ("relu",)), ("bf16", 512, 7, ("relu", "cl plane")), ("f32", 2048, 7, ("none", "add_relu")),
                                     ("bf16", 2048, 7, ("none", "add_relu")))]
BN7_BWD = [("bn_bwd", c, 3) for c in (("f32", 512, 7, 1), ("bf16", 512, 7, 1), ("f32", 2048, 7, 3), ("f32", 2048, 7, 0), ("bf16", 2048, 7, 3),
                                     ("bf16", 2048, 7, 0))]


def entry(switch, value, relation, why, cases=(), names=(), trainer=None, base=None):
    return dict(switch=switch, value=value, key="%s=%s" % (switch, value), relation=relation, why=why, cases=list(cases), names=list(names),
                trainer=trainer, base=dict(base or {}))


ROUTES = [
    # ---- bf16 NCHW kernels (kernels_igemm_bf16.hip): bgemm_kernel<op, k, s, bm, vw [, swp] [, sbuf]> ----
    entry("RESNET_MI_BF16_VW", "1", "bounds", "element-wise gathers, channel-major product with the LDS-transpose epilogue: another accumulator layout",
          convs(BF, ALL, [S_3x3, S_1x1_whole, S_3x3s2]) + convs(BF, FD, [S_49]) + [conv_bn(BF, S_3x3)],
          ["bgemm_kernel<fwd,k3,s1,bm64,vw1>", "bgemm_kernel<dgrad,k3,s1,bm64,vw1>", "bgemm_kernel<wgrad,k3,s1,bm128,vw1>",
           "bgemm_kernel<fwd,k1,s1,bm64,vw1>", "bgemm_kernel<dgrad,k1,s1,bm64,vw1>", "bgemm_kernel<wgrad,k1,s1,bm128,vw1>",
           "bgemm_kernel<fwd,k3,s2,bm64,vw1>", "bgemm_kernel<dgrad,k3,s2,bm64,vw1>", "bgemm_kernel<wgrad,k3,s2,bm128,vw1>"]),
    entry("RESNET_MI_BF16_VW", "4", "bounds", "weight gradient staged 4 pixels per load: the k-steps hold other pixels (padding to groups of 4, not 8)",
          convs(BF, ("wgrad",), [S_3x3, S_1x1_whole, (128, 16, 128, 3, 2, 3)]),
          ["bgemm_kernel<wgrad,k3,s1,bm128,vw4>", "bgemm_kernel<wgrad,k1,s1,bm128,vw4>", "bgemm_kernel<wgrad,k3,s2,bm128,vw4>"]),
    entry("RESNET_MI_BF16_SWP", "0", "bounds", "channel-major product instead of the pixel-major one: another accumulator layout and statistics tree",
          convs(BF, FD, [S_3x3, S_1x1, S_1x1_whole]) + [conv(BF, "fwd", S_3x3s2), conv_bn(BF, S_3x3), conv_bn(BF, S_1x1_whole)],
          ["bgemm_kernel<fwd,k3,s1,bm64,vw8>", "bgemm_kernel<dgrad,k3,s1,bm64,vw8>", "bgemm_kernel<fwd,k1,s1,bm64,vw8>",
           "bgemm_kernel<dgrad,k1,s1,bm64,vw8>", "bgemm_kernel<fwd,k3,s2,bm64,vw8>"]),
    entry("RESNET_MI_BF16_SBUF", "1", "bitwise", "one operand buffer: the same k-steps in the same order",
          convs(BF, FD, [S_3x3, S_1x1, S_1x1_whole]) + [conv(BF, "fwd", S_3x3s2), conv_bn(BF, S_3x3), dgrad_bn(BF, S_1x1, "red")],
          ["bgemm_kernel<fwd,k3,s1,bm64,vw8,swp,sbuf>", "bgemm_kernel<dgrad,k3,s1,bm64,vw8,swp,sbuf>", "bgemm_kernel<fwd,k1,s1,bm64,vw8,swp,sbuf>",
           "bgemm_kernel<dgrad,k1,s1,bm64,vw8,swp,sbuf>", "bgemm_kernel<fwd,k3,s2,bm64,vw8,swp,sbuf>"]),
    # 540 / 588 tiles: more than 512 slots, at most 768 -- the planner takes one buffer there
    entry("RESNET_MI_BF16_SBUF", "0", "bitwise", "two operand buffers: the same k-steps in the same order",
          [conv(BF, "fwd", (64, 56, 256, 1, 1, 11)), conv(BF, "fwd", (64, 56, 256, 1, 1, 12)), conv(BF, "dgrad", (256, 56, 64, 1, 1, 11)),
           conv_bn(BF, (64, 56, 256, 1, 1, 11))],
          ["bgemm_kernel<fwd,k1,s1,bm128,vw8,swp>", "bgemm_kernel<dgrad,k1,s1,bm128,vw8,swp>"]),
    # (M / 128) * column tiles >= 256: the planner takes 128 rows there (as 64-row tiles the 56 x 56 cases are 588 tiles: one buffer)
    entry("RESNET_MI_BF16_BM", "64", "bounds", "64-row tiles: four statistics partials per column tile instead of two",
          [conv(BF, "fwd", (512, 7, 2048, 1, 1, 35)), conv(BF, "fwd", (64, 56, 256, 1, 1, 6)), conv(BF, "dgrad", (256, 56, 64, 1, 1, 6)),
           conv(BF, "dgrad", (2048, 7, 512, 1, 1, 35)), conv_bn(BF, (64, 56, 256, 1, 1, 6)), dgrad_bn(BF, (256, 56, 64, 1, 1, 6))],
          ["bgemm_kernel<fwd,k1,s1,bm64,vw8>", "bgemm_kernel<fwd,k1,s1,bm64,vw8,swp,sbuf>", "bgemm_kernel<dgrad,k1,s1,bm64,vw8,swp,sbuf>",
           "bgemm_kernel<dgrad,k1,s1,bm64,vw8>"]),
    entry("RESNET_MI_BF16_BM", "128", "bounds", "128-row tiles: two statistics partials per column tile instead of four",
          convs(BF, FD, [S_3x3, S_1x1, S_49]) + [conv(BF, "fwd", S_1x1_whole), conv(BF, "fwd", S_3x3s2), conv_bn(BF, S_3x3), dgrad_bn(BF, S_1x1, "red")],
          ["bgemm_kernel<fwd,k3,s1,bm128,vw8,swp>", "bgemm_kernel<dgrad,k3,s1,bm128,vw8,swp>", "bgemm_kernel<fwd,k1,s1,bm128,vw8,swp>",
           "bgemm_kernel<dgrad,k1,s1,bm128,vw8,swp>", "bgemm_kernel<fwd,k3,s1,bm128,vw8>", "bgemm_kernel<dgrad,k3,s1,bm128,vw8>",
           "bgemm_kernel<fwd,k3,s2,bm128,vw8,swp>"]),
    entry("RESNET_MI_BF16_PW_WGRAD", "0", "bounds", "the NCHW kernel instead of the LDS-DMA one: another k-split and tile order",
          convs(BF, ("wgrad",), [S_1x1, (128, 14, 256, 1, 1, 3)]), ["bgemm_kernel<wgrad,k1,s1,bm128,vw8>"]),
    # ---- bf16 channel-last kernel (kernels_cl_bf16.hip): cl_conv_kernel<taps, bm, nbuf> ----
    entry("RESNET_MI_CL_NBUF", "1", "bitwise", "one operand buffer and two barriers per k-step: the same k-steps in the same order",
          convs(BF, FD, [(64, 8, 64, 3, 1, 4), S_3x3], "cl") + [conv(BF, "fwd", (128, 8, 128, 3, 2, 4), "cl"), conv_bn(BF, S_3x3, "cl")],
          ["cl_conv_kernel<taps9,bm64,nbuf1>", "cl_conv_kernel<taps9,bm128,nbuf1>"]),
    # ---- split reduce of the weight gradients (kernels_igemm.hip) ----
    # N = 8 is the smallest of 4, 8, 16, 33 at which a ResNet-50 1x1 layer's default plan is grouped (256 -> 64 @56: 16 splits; the 3x3 64 -> 64 @56 as well)
    entry("RESNET_MI_WGRAD_REDUCE_G", "0", "bounds", "one thread sums all splits of an output in ascending order instead of 8 groups and a tree",
          [conv(F32, "wgrad", (256, 56, 64, 1, 1, 8)), conv(F32, "wgrad", (64, 56, 64, 3, 1, 8))],
          ["igemm_wgrad_reduce_kernel<k1,flat>", "igemm_wgrad_reduce_kernel<k3,flat>"]),
    # ---- batch norm, element-wise passes (kernels_bn.hip): bn_apply_kernel / bn_bwd_apply_kernel<x type, activation type, v [, straddle]> ----
    entry("RESNET_MI_BN_STRADDLE", "0", "bitwise", "one element per thread instead of vectors that straddle planes: the same arithmetic per element",
          BN7_FWD + BN7_BWD,
          ["bn_apply_kernel<f32,f32,v1>", "bn_apply_kernel<bf16,bf16,v1>", "bn_bwd_apply_kernel<f32,f32,v1>", "bn_bwd_apply_kernel<bf16,bf16,v1>"]),
    # ---- fp32 implicit GEMM (kernels_igemm.hip): igemm_kernel<op, k, s, bm [, vb] [, tail]> ----
    # 19 x 49 and 32 x 196 columns: the planner takes 128 rows there (32 x 196 = 49 whole tiles)
    entry("RESNET_MI_IGEMM_BM", "64", "bounds", "64-row tiles: other tail slices, four statistics partials per column tile",
          convs(F32, FD, [(512, 7, 512, 3, 1, 19), (256, 14, 256, 3, 1, 32)]) + [conv(F32, "fwd", (64, 56, 256, 1, 1, 8)), conv_bn(F32, (512, 7, 512, 3, 1, 19))],
          ['igemm_kernel<fwd,k3,s1,bm64,tail>', 'igemm_kernel<dgrad,k3,s1,bm64,tail>', 'igemm_kernel<fwd,k1,s1,bm64,vb>']),
    entry("RESNET_MI_IGEMM_BM", "128", "bounds", "128-row tiles: other tail slices, two statistics partials per column tile",
          convs(F32, FD, [S_3x3, S_1x1, S_49]) + [conv(F32, "fwd", S_1x1_whole), conv(F32, "fwd", S_3x3s2), conv_bn(F32, S_3x3), dgrad_bn(F32, S_1x1, "red")],
          ['igemm_kernel<fwd,k3,s1,bm128,tail>', 'igemm_kernel<dgrad,k3,s1,bm128,tail>', 'igemm_kernel<fwd,k1,s1,bm128,vb>', 'igemm_kernel<dgrad,k1,s1,bm128,vb>', 'igemm_kernel<fwd,k3,s2,bm128,tail>']),
    entry("RESNET_MI_IGEMM_TAIL", "0", "bounds", "no reduction-sliced tail round: every tile sums its whole reduction in one workgroup",
          convs(F32, FD, [S_3x3, S_49]) + [conv(F32, "fwd", S_3x3s2), conv_bn(F32, S_3x3)],
          ['igemm_kernel<fwd,k3,s1,bm64>', 'igemm_kernel<dgrad,k3,s1,bm64>', 'igemm_kernel<fwd,k3,s2,bm64>']),
    # ---- direct VALU kernels (kernels_conv.hip, the route of every fp32 shape that does not tile; here under RESNET_MI_IGEMM=0, and compared
    # with a child that sets only that): dconv_kernel<taps, tk, jm, cc [, class ...]> ----
    entry("RESNET_MI_DCONV_LDS", "1024", "bitwise", "smaller channel chunks in LDS: every output still sums channels and taps in ascending order",
          D_CASES, ["dconv_kernel<t3x3,tk32,jm2,cc2>", "dconv_kernel<t3x3,tk32,jm2,cc3>"], base=DIRECT),
    entry("RESNET_MI_DCONV_TK", "16", "bitwise", "16 output channels per thread: each output's own sum is unchanged",
          D_CASES, ["dconv_kernel<t3x3,tk16,jm2,cc8>", "dconv_kernel<t7x7,tk16,jm7,cc1>"], base=DIRECT),
    entry("RESNET_MI_DCONV_TK", "64", "bitwise", "64 output channels per thread: each output's own sum is unchanged",
          D_CASES, ["dconv_kernel<t3x3,tk64,jm2,cc8>", "dconv_kernel<t7x7,tk64,jm7,cc1>"], base=DIRECT),
    # 4 x 16 pixels per parity class: part of one workgroup; 28 x 16 = 448: one whole workgroup
    entry("RESNET_MI_DGRAD_STREAMS", "0", "bitwise", "the four parity classes of a stride-2 dgrad in series on one stream: the same four launches",
          convs(F32, ("dgrad",), [(128, 8, 128, 3, 2, 4), (64, 8, 64, 3, 2, 28)]),
          ["dconv_kernel<t2x2,tk32,jm2,cc8,class in series>", "dconv_kernel<t1x1,tk32,jm2,cc8,class in series>"], base=DIRECT),
    # ---- trainer-level switches: whole steps (test_trainer_under_switch) ----
    entry("RESNET_MI_IGEMM", "0", "bounds", "every convolution off the matrix cores: VALU stem, no fused statistics, no BN' fusion", trainer=F32),
    entry("RESNET_MI_IGEMM", "1", "bounds", "1x1 forward / dgrad on gemm_mfma_kernel, 3x3 on the direct kernels", trainer=F32),
    entry("RESNET_MI_F32_BNFUSE_BWD", "0", "bounds", "no dgrad carries a BN' reduction: bn_bwd_reduce_kernel's tree instead of the epilogue's", trainer=F32),
    entry("RESNET_MI_F32_BNFUSE_BWD", "1", "bounds", "the expansion dgrads carry the BN' reduction", trainer=F32),
    entry("RESNET_MI_F32_BNFUSE_BWD", "2", "bounds", "the spatial dgrads carry the BN' reduction", trainer=F32),
    entry("RESNET_MI_F32_BNFUSE_BWD", "7", "bounds", "every site's dgrad carries the BN' reduction", trainer=F32),
    entry("RESNET_MI_STEM_MFMA", "0", "bounds", "the fp32 stem on the direct kernels: another summation order, statistics by a pass of their own", trainer=F32),
    entry("RESNET_MI_PRELAYOUT", "0", "bitwise", "each convolution re-lays its own weights: the same values in the same layout", trainer=F32),
    entry("RESNET_MI_OVERLAP", "0", "bitwise", "weight gradients on the compute stream: a schedule of the same kernels", trainer="both"),
    entry("RESNET_MI_OVERLAP", "2", "bitwise", "free-running weight gradients over the ring of derivative buffers (bf16: falls back to mode 1)", trainer="both"),
    entry("RESNET_MI_BF16_CL_S1_DGRAD", "0", "bounds", "stride-1 3x3 dgrads on the NCHW kernels", trainer=BF),
    entry("RESNET_MI_BF16_STEM", "0", "bounds", "the bf16 trainer's stem on the fp32 direct kernels", trainer=BF),
]

# the switches test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes re-runs the bf16 whole-step checks under: the four it
# always had, and the table's bf16 trainer entries
BF16_TRAINER_SWITCHES = ["RESNET_MI_BF16_CL_S2=0", "RESNET_MI_BF16_CL_S1=0", "RESNET_MI_BF16_CL_DGRAD2=0", "RESNET_MI_BF16_STEM_TENSORS=f32"] + \
    [e["key"] for e in ROUTES if e["trainer"] == BF and e["relation"] == "bounds"]

# switches that select no kernel, or that another test pins
EXEMPT = {
    "RESNET_MI_TRACE": "diagnostic: records launch names (the ring these tests read), selects nothing",
    "RESNET_MI_LDS_FILL": "test aid: a word into all LDS after every launch (tests/test_gpu_lds.py runs the table's operator cases under it); selects nothing",
    "RESNET_MI_LIB": "which build of the library binding.py loads (tools/variant.sh), not a route inside it",
    "RESNET_MI_BNFUSE": "pinned by test_gpu_net.py::test_fused_bn_statistics_match_separate_pass (a child process per value)",
    "RESNET_MI_BF16_BNFUSE_BWD": "pinned by test_gpu_bf16.py::test_resnet50_bf16_every_block_and_both_bn_backward_routes (a trainer per value)",
    "RESNET_MI_BF16_CL_S1": "pinned by test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes",
    "RESNET_MI_BF16_CL_S2": "pinned by test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes",
    "RESNET_MI_BF16_CL_DGRAD2": "pinned by test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes",
    "RESNET_MI_BF16_STEM_TENSORS": "pinned by test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes",
}


def by_key(key):
    return next(e for e in ROUTES if e["key"] == key)


def env_of(e):
    """the child's environment additions: the entry's base (the route its default is taken on) and the switch itself"""
    return dict(e["base"], **{e["switch"]: e["value"]})


def case_id(case):
    return repr(case)


def union_cases(entries):
    """the cases of several entries, each once, in table order"""
    seen, out = set(), []
    for e in entries:
        for c in e["cases"]:
            if case_id(c) not in seen:
                seen.add(case_id(c))
                out.append(c)
    return out
