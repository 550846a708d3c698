"""The mutant table of tests/test_gpu_mutants.py: one small VALUE fault per entry, planted in a copy of one source file under
resnet_amd/csrc, built as a second library (tools/build_mutants.py -> variants/mutants/libresnet_mi_<name>.so) and loaded through
RESNET_MI_LIB.  The entry's killers -- existing checks of the suite that reach the mutated branch -- must fail on that library.

The value-only rule ("Suite sensitivity"): a mutant changes a value that is stored or accumulated (a constant, a dropped term,
a comparison that selects between two values, a rounding, a factor of 0 on one contribution).  It never changes an address, an index, a
loop bound, a barrier or a wait, a launch geometry, an LDS or buffer size, a *_supported predicate, or a value later code uses as an
address or a bound; no `old` or `new` holds inline assembly.  "Skip the last slice" is "multiply the last slice by 0".

name     unique; the library is libresnet_mi_<name>.so
file     under resnet_amd/csrc; `old` occurs exactly once in it
what     the fault and which elements it makes wrong
branch   the code path the fault lives in (the kill matrix of DESIGN.md)
killers  pytest node ids, one to three, the smallest cases that reach the branch; the planner's answer (convref.conv_plan:
         rows per tile, columns per tile, tiles, first sliced tile, slices, splits, grouped) stands beside the cases that were chosen for it
"""

RAG = "tests/test_gpu_ragged.py::"
OPS = "tests/test_gpu_ops.py::"
BF = "tests/test_gpu_bf16.py::"
MIX = "tests/test_gpu_mix.py::"
EMA = "tests/test_gpu_ema.py::"
ACC = "tests/test_gpu_accum.py::"
LOSS = "tests/test_gpu_loss_head.py::"
AA = "tests/test_gpu_input_aa.py::"

MUTANTS = []


def _m(name, file, old, new, what, branch, killers):
    MUTANTS.append(dict(name=name, file=file, old=old, new=new, what=what, branch=branch, killers=list(killers)))


# ---------------------------------------------------------------------------------------------------------------------------
# kernels_igemm.hip
_m("igemm_tail_last_slice", "kernels_igemm.hip",
   "for (int i = 0; i < 8; i++) v[i] += tb[(size_t)z * (BM * 128) + i * 128];",
   "for (int i = 0; i < 8; i++) v[i] += (z == g.tsplit - 1 ? 0.f : 1.f) * tb[(size_t)z * (BM * 128) + i * 128];",
   "igemm_tail_reduce_kernel multiplies the last reduction slice by 0: every element of a sliced tail tile lacks that slice's terms",
   "sliced tail tiles only",
   # plan (64, 128, 2, 0, 2, 1, 0): both tiles are cut into 2 slices; dgrad (64, 128, 2, 0, 2, 1, 0)
   [RAG + "test_conv_route_ragged[c1s_N4-f32_default_fwd_C64_H8_K64_k3_s1]",
    RAG + "test_conv_route_ragged[c1s_N4-f32_default_dgrad_C128_H4_K512_k1_s1]"])
_m("igemm_fwd_m2_mean_shift", "kernels_igemm.hip",
   "g.bn_part[2 * plane + o] = fmaxf(sq - sd * sd * inv, 0.f);\n    }\n    IG_T(4);",
   "g.bn_part[2 * plane + o] = fmaxf(sq, 0.f);\n    }\n    IG_T(4);",
   "the forward epilogue's BN partial keeps the sum of squares about the tile's first column as M2 (drops the mean-shift term): the "
   "variances of every channel come out too large",
   "unsliced forward tiles with fused statistics",
   # plan (64, 128, 2, 2, 1, 1, 0): two whole tiles, no slices
   [RAG + "test_conv_bn_fwd_ragged[c1s_N4-f32_C64_H8_K64_k1_s1]"])
_m("igemm_dgrad_addend_rows64", "kernels_igemm.hip",
   "if (MODE == IG_DGRAD && addend) v += ad[r];",
   "if (MODE == IG_DGRAD && addend) v += (wm > 0 ? 0.f : ad[r]);",
   "the dgrad epilogue ignores the shortcut addend in rows 64..127 of a 128-row tile",
   "128-row tiles (waves with wm = 1), dgrad with an addend",
   # plan (128, 128, 392, 392, 1, 1, 0): 128-row tiles; "stage 1 red" takes the shortcut gradient as its addend
   [RAG + "test_conv_route_ragged[r50_N8-f32_default_dgrad_C256_H56_K64_k1_s1]"])
_m("igemm_wgrad_reduce_remainder", "kernels_igemm.hip",
   "for (; z < splits; z++)\n#pragma unroll\n        for (int t = 0; t < T; t++) s[t] += part[((long)z * T + t) * KC + i];",
   "for (; z < splits; z++)\n#pragma unroll\n        for (int t = 0; t < T; t++) s[t] += 0.f * part[((long)z * T + t) * KC + i];",
   "igemm_wgrad_reduce_kernel multiplies by 0 the splits behind the last whole group of U (8 for 1x1): dW lacks those splits' pixels",
   "the remainder loop of the flat split reduction (splits % 8 != 0)",
   # plan (128, 128, 2, 2, 1, 12, 0): 12 splits, flat reduction: splits 8..11 are the remainder
   [RAG + "test_conv_route_ragged[r50_N8-f32_default_wgrad_C256_H56_K128_k1_s1]"])

# kernels_conv.hip (the direct kernels: by default only shapes whose channel counts do not tile for the implicit GEMM reach them)
_m("dconv_tap22_zero", "kernels_conv.hip",
   "for (int t = 0; t < TK; t++) acc[t] = fmaf(wq[t], v, acc[t]);",
   "for (int t = 0; t < TK; t++) acc[t] = fmaf((NTR == 3 && NTC == 3 && tr == 2 && tc == 2) ? 0.f : wq[t], v, acc[t]);",
   "the direct 3x3 kernel reads the weight of tap (2, 2) as 0: every output lacks one of its nine taps",
   "the 3x3 instantiation of dconv_kernel",
   [OPS + "test_direct_kernels_per_element[fwd_C64_H8_K96_k3_s1_N2]"])
_m("dconv_s2_dgrad_odd_odd_scale", "kernels_conv.hip",
   "for (int t = 0; t < TK; t++) acc[t] = fmaf(wq[t], v, acc[t]);",
   "for (int t = 0; t < TK; t++) acc[t] = fmaf((NTR == 2 && NTC == 2) ? wq[t] * 1.0009765625f : wq[t], v, acc[t]);",
   "the (odd row, odd column) parity class of the direct stride-2 dgrad is scaled by 1 + 2^-10: a quarter of dx",
   "the 2x2-tap parity class of the stride-2 dgrad",
   [OPS + "test_direct_kernels_per_element[dgrad_C32_H8_K64_k3_s2_N3]"])
_m("dconv_wgrad_image1_zero", "kernels_conv.hip",
   "d[u][q4] = ok ? v : 0.f;",
   "d[u][q4] = (ok && g.n != 1) ? v : 0.f;",
   "the direct weight gradient multiplies image 1's contribution by 0",
   "one image of the reduction",
   [OPS + "test_direct_kernels_per_element[wgrad_C96_H14_K128_k3_s1_N2]"])

# kernels_gemm.hip
_GEMM_OLD = "acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);"
_m("gemm_nn_last_k", "kernels_gemm.hip", _GEMM_OLD,
   "acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32((BATCH == BATCH_NONE && A_KC && !B_KC && k0 + k2 + fk == g.K - 1) ? 0.f : av[cur][i], "
   "bv[cur][j], acc[i][j], 0, 0, 0);",
   "the plain product A B (the FC forward) takes the last reduction element's product as 0",
   "one instantiation (BATCH_NONE, A k-contiguous, B n-contiguous), last k",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-fc_nn]"])
_m("gemm_rows64_last_k", "kernels_gemm.hip", _GEMM_OLD,
   "acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32((wm > 0 && k0 + k2 + fk == kend - 1) ? 0.f : av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);",
   "rows 64..127 of a 128-row tile lose the product of their last reduction element (X^T dY, the FC weight gradient, is the form with "
   "more than 64 rows)",
   "128-row tiles (waves with wm = 1), last k",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-fc_lt]"])

# kernels_igemm_bf16.hip
_m("bgemm_bn_bwd_unrounded_sums", "kernels_igemm_bf16.hip",
   "const float g0 = on0 ? __uint_as_float(pk[e] << 16) : 0.f, g1 = on1 ? __uint_as_float(pk[e] & 0xffff0000u) : 0.f;",
   "const float g0 = on0 ? w[2 * e] : 0.f, g1 = on1 ? w[2 * e + 1] : 0.f;",
   "the fused BN' epilogue sums the gradient before its rounding to bf16 (the contract sums the stored one): dbeta, dgamma and the dx "
   "made from them",
   "the BN'-fused dgrad epilogue (pixel-major product)",
   [RAG + "test_dgrad_bn_bwd_ragged[c1s_N4-bf16_C64_H8_K256_k1_s1]", RAG + "test_dgrad_bn_bwd_ragged[c4i_N4-bf16_C256_H8_K128_k1_s1]"])
_m("bgemm_bn_bwd_gate_ge", "kernels_igemm_bf16.hip",
   "const bool on0 = (int16_t)(mv[e] & 0xffffu) > 0,",
   "const bool on0 = (int16_t)(mv[e] & 0xffffu) >= 0,",
   "the gate of the BN'-fused dgrad is mask >= 0 on the even pixels: the gradient passes where the activation is 0",
   "the BN'-fused dgrad epilogue, even pixels",
   [RAG + "test_dgrad_bn_bwd_ragged[c1s_N4-bf16_C64_H8_K256_k1_s1]"])
_m("bgemm_fwd_stats_count_padding", "kernels_igemm_bf16.hip",
   "if (col < g.ncols && pp < (uint32_t)g.P) { okm |= 1u << (j * 4 + q); cnt += 4; }",
   "if (col < g.ncols && pp < (uint32_t)g.P) okm |= 1u << (j * 4 + q);\n                if (col < g.ncols) cnt += 4;",
   "the forward statistics partial counts the padding columns of Pc (planes that are no multiple of 8 pixels) in n: means and variances "
   "of every channel",
   "planes with P % 8 == 4 (14 x 14: Pc = 200), pixel-major epilogue",
   # plan (64, 128, 52, 52, 1, 1, 0)-like: P = 196, Pc = 200
   [RAG + "test_conv_bn_fwd_ragged[r50_N8-bf16_C1024_H14_K256_k1_s1]"])
_m("bgemm_f2b_truncates", "kernels_igemm_bf16.hip",
   "out[i] = bg_f2bf(in[i]);",
   "out[i] = (u16)(__float_as_uint(in[i]) >> 16);",
   "the fp32 -> bf16 conversion kernel truncates instead of rounding to the nearest even",
   "bg_f2b_kernel",
   [BF + "test_conversion_is_round_to_nearest_even"])

# kernels_cl_bf16.hip
_m("cl_fwd_stats_past_the_end", "kernels_cl_bf16.hip",
   "const float dlt = col < g.ncols ? acc[i][j][r] - s0 : 0.f;",
   "const float dlt = acc[i][j][r] - s0;",
   "the channel-last forward's statistics partial of the partial last column tile sums the columns past the end as well",
   "the partial last column tile",
   # 8 x 196 = 1568 columns = 24.5 waves of 64: the last wave holds 32 real columns and 32 past the end.  (The small nets' 64 columns
   # end ON a wave boundary: a wave that lies wholly past the end sees 64 copies of the last pixel, d = 0 for each of them, and the
   # mutant writes the same bits -- it survived c1s_N4-bf16_cl_C128_H4_K128_k3_s1 and ..._C128_H8_K128_k3_s2)
   [RAG + "test_conv_bn_fwd_ragged[r50_N8-bf16_cl_C256_H28_K256_k3_s2]"])
_m("cl_dgrad2_odd_column_ulp", "kernels_cl_bf16.hip",
   "u32x4 v = {cl_pack2(acc[0][i][j][4 * q], acc[1][i][j][4 * q]),",
   "u32x4 v = {cl_pack2(acc[0][i][j][4 * q], acc[1][i][j][4 * q] * 1.0078125f),",
   "cl_dgrad2_kernel scales the odd column parity of every fourth grid pixel by 1 + 2^-7, one bf16 ulp",
   "odd output columns",
   [RAG + "test_conv_route_ragged[c1s_N4-bf16_cl_dgrad_C128_H8_K128_k3_s2]"])
_m("cl_wgrad2_last_split", "kernels_cl_bf16.hip",
   "            compute((it - r_beg) & 1);\n        }\n    }\n"
   "    float *o = part + ((size_t)((size_t)split * 9 + t) * g.K) * g.C + c0 + wn * 64 + (lane & 31);\n"
   "#pragma unroll\n    for (int i = 0; i < 2; i++)\n#pragma unroll\n        for (int j = 0; j < 2; j++)\n#pragma unroll\n"
   "            for (int r = 0; r < 16; r++)\n"
   "                o[(size_t)(m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * g.C + j * 32] = acc[i][j][r];",
   "            compute((it - r_beg) & 1);\n        }\n    }\n"
   "    float *o = part + ((size_t)((size_t)split * 9 + t) * g.K) * g.C + c0 + wn * 64 + (lane & 31);\n"
   "    const float keep = (r_beg > 0 && r_end == g.rtiles) ? 0.f : 1.f;\n"
   "#pragma unroll\n    for (int i = 0; i < 2; i++)\n#pragma unroll\n        for (int j = 0; j < 2; j++)\n#pragma unroll\n"
   "            for (int r = 0; r < 16; r++)\n"
   "                o[(size_t)(m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * g.C + j * 32] = keep * acc[i][j][r];",
   "cl_wgrad2_kernel multiplies its last split's partial by 0 (where there is more than one split)",
   "the last reduction split",
   # plan (128, 128, 9, 9, 1, 4, 0): 4 splits
   [RAG + "test_conv_route_ragged[r50_N8-bf16_cl2_wgrad_C128_H56_K128_k3_s2]"])
_m("pw_wgrad_last_split", "kernels_cl_bf16.hip",
   "    // partials [split][k][c]\n    float *o = part + ((size_t)split * g.K) * g.C + c0 + wn * 64 + (lane & 31);\n"
   "#pragma unroll\n    for (int i = 0; i < 2; i++)\n#pragma unroll\n        for (int j = 0; j < 2; j++)\n#pragma unroll\n"
   "            for (int r = 0; r < 16; r++)\n"
   "                o[(size_t)(m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * g.C + j * 32] = acc[i][j][r];",
   "    // partials [split][k][c]\n    float *o = part + ((size_t)split * g.K) * g.C + c0 + wn * 64 + (lane & 31);\n"
   "    const float keep = (r_beg > 0 && r_end == g.rtiles) ? 0.f : 1.f;\n"
   "#pragma unroll\n    for (int i = 0; i < 2; i++)\n#pragma unroll\n        for (int j = 0; j < 2; j++)\n#pragma unroll\n"
   "            for (int r = 0; r < 16; r++)\n"
   "                o[(size_t)(m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * g.C + j * 32] = keep * acc[i][j][r];",
   "the 1x1 LDS-DMA weight gradient (pw_wgrad_kernel) multiplies its last split's partial by 0",
   "the last reduction split",
   # plan (128, 128, 4, 4, 1, 6, 0): 6 splits
   [RAG + "test_conv_route_ragged[r50_N8-bf16_pw_wgrad_C128_H28_K512_k1_s1]"])

# kernels_stem_bf16.hip
_m("stem_fwd_tap66_zero", "kernels_stem_bf16.hip",
   "if (s >= 0) v = w[(size_t)k * 147 + gq * 7 + s]; // KCRS",
   "if (s >= 0 && !(gq % 7 == 6 && s == 6)) v = w[(size_t)k * 147 + gq * 7 + s]; // KCRS",
   "the bf16 stem forward reads tap (6, 6) of every input channel as 0",
   "one of 49 taps (the forward weight operand)",
   [RAG + "test_stem_ragged[c1s_N4-bf16_fwd]"])
_m("stem_exact_image_rounded", "kernels_stem_bf16.hip",
   "        xp[e] = v;\n",
   "        xp[e] = mi_bf2f(mi_f2bf(v));\n",
   "the exact-fp32 stem pair rounds the image to bf16 when it pads it into parity planes: forward and weight gradient",
   "st32_pad_kernel",
   [RAG + "test_stem_ragged[c1s_N4-f32_wgrad]", RAG + "test_stem_ragged[c1s_N4-f32_fwd]"])
_m("stem_wgrad_reduce_remainder", "kernels_stem_bf16.hip",
   "for (; w < nwaves; w += 4) s[0] += p[(size_t)w * WS];",
   "for (; w < nwaves; w += 4) s[0] += 0.f * p[(size_t)w * WS];",
   "st_wgrad_reduce_kernel multiplies by 0 the partials behind the last whole group of 32 waves",
   "the remainder loop of the stem's weight-gradient reduction",
   # waves = min(N P / 16, 1024) rounded up to 4: 64 at N = 4, H = 32 and 1024 at H = 224 are multiples of 32 (no remainder: the mutant
   # survived c1s_N4-bf16_wgrad); 144 at N = 1, H = 96 leaves 16 waves to the remainder loop
   [BF + "test_stem_bf16[96-1]"])

# kernels_bn.hip
_m("bn_wel_merge_between_term", "kernels_bn.hip",
   "r.m2 = a.m2 + b.m2 + d * d * a.n * f;",
   "r.m2 = a.m2 + b.m2;",
   "wel_merge drops d*d*a.n*f, the between-group term of M2: every variance is too small",
   "every merge of two partial statistics",
   [RAG + "test_bn_fwd_ragged[c1s_N4-f32_C64_H8]"])
_m("bn_apply_no_eps", "kernels_bn.hip",
   "sd0 = sqrtf(vars[c] + eps), g0 = gamma[c], b0 = beta[c];\n        int nfirst = V;",
   "sd0 = sqrtf(vars[c]), g0 = gamma[c], b0 = beta[c];\n        int nfirst = V;",
   "bn_apply_kernel divides by sqrtf(var) without eps: channels of small variance",
   "the apply kernel (the statistics and the backward keep eps)",
   [RAG + "test_bn_fwd_ragged[c1s_N4-f32_C256_H8]", RAG + "test_bn_fwd_ragged[c1s_N4-f32_C64_H8]"])
_m("bn_apply_straddle_beta", "kernels_bn.hip",
   "b1 = beta[c1];\n        }",
   "b1 = b0;\n        }",
   "in a vector that straddles two channel planes the second channel's elements take the first channel's beta",
   "the straddling vectors of 7 x 7 planes (STR)",
   [RAG + "test_bn_fwd_ragged[r50_N8-f32_C512_H7]"])
_m("bn_bwd_dx_no_mean_dy", "kernels_bn.hip",
   "xv[q] = scale * (gq - k1 - xh * k2);",
   "xv[q] = scale * (gq - xh * k2);",
   "the backward dx drops the mean(dy) term",
   "bn_bwd_apply_kernel",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C256_H8_mode0]"])
_m("bn_bwd_gate_ge", "kernels_bn.hip",
   "if (EXT) on = m > 0.f;",
   "if (EXT) on = m >= 0.f;",
   "the external-mask gate of the BN backward reduction is mask >= 0: the gated gradient and the sums take dy where the activation is 0",
   "the external-mask modes (2, 3) of bn_bwd_reduce_kernel",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C256_H8_mode3]"])
_m("bn_bwd_gate_y_ge", "kernels_bn.hip",
   "if (MASK == 1) on = bn_y(xh, g, b) > 0.f;\n        if (EXT) on = m > 0.f;",
   "if (MASK == 1) on = bn_y(xh, g, b) >= 0.f;\n        if (EXT) on = m > 0.f;",
   "the recomputed gate of the BN backward reduction is y >= 0: dbeta and dgamma take dy where y is exactly 0",
   "mode 1 of bn_bwd_reduce_kernel, elements with y == 0 (x == mean in a beta == 0 channel)",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C64_H8_mode1]"])
_m("bn_running_biased_var", "kernels_bn.hip",
   "m * (e.vars[c] * e.unbias);",
   "m * (e.vars[c]);",
   "bn_running_update_kernel folds the biased batch variance into the running variance",
   "the running-variance half of the arena",
   ["tests/test_gpu_eval.py::test_running_update_kernel[momentum_0.1]"])
_m("bn_sync_no_between_replica", "kernels_bn.hip",
   "tmp[c] = vars[c] + d * d;",
   "tmp[c] = vars[c];",
   "the sync-BN merge drops the between-replica mean term of the variance",
   "bn_sync_k2",
   ["tests/test_gpu_dp.py::test_sync_bn_merge_of_two_different_replicas_equals_the_whole_batch[shape0]"])

# kernels_misc.hip
_m("softmax_no_max", "kernels_misc.hip",
   "    mx = wave_max(mx);\n    float s = 0.f;\n    for (int j = lane; j < L; j += 64) s += expf(xr[j] - mx);",
   "    mx = 0.f * wave_max(mx);\n    float s = 0.f;\n    for (int j = lane; j < L; j += 64) s += expf(xr[j] - mx);",
   "the soft-max does not subtract the row maximum: rows with logits past +-88 overflow or vanish",
   "rows with large logits",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-softmax_ce_deriv]"])
_m("adam_v_corrected_with_beta1", "kernels_misc.hip",
   "va = vi / (1.f - cur_b2);",
   "va = vi / (1.f - cur_b1);",
   "Adam corrects the second moment with beta1^t",
   "every element",
   [OPS + "test_softmax_ce_adam"])
_m("adam_m_on_nan_gradient", "kernels_misc.hip",
   "if (isnan(gi) || isinf(gi)) b = true;",
   "if (isnan(gi) || isinf(gi)) { b = true; m[i] = b1 * mi + (1.f - b1) * gi; }",
   "Adam updates m from a NaN / Inf gradient (the guard keeps the old moments)",
   "elements with a non-finite gradient",
   [OPS + "test_softmax_ce_adam"])
_m("maxpool_last_of_equal_maxima", "kernels_misc.hip",
   "if (e > mv[j]) { mv[j] = e;",
   "if (e >= mv[j]) { mv[j] = e;",
   "the 3x3 stride-2 max-pool takes the last of equal maxima inside a window (the index stays in the window)",
   "windows with ties",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-maxpool_f32]"])
_m("avgpool_bwd_divisor", "kernels_misc.hip",
   "stf<T>(dx + e, dy[e / P] / (float)P);",
   "stf<T>(dx + e, dy[e / P] / (float)(P + 1));",
   "the average-pool backward divides by H^2 + 1",
   "every element",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-avgpool_f32]"])
_m("misc_bf16_store_truncates", "kernels_misc.hip",
   "{ *p = mi_f2bf(v); }",
   "{ *p = (bf16_t)(__float_as_uint(v) >> 16); }",
   "the pooling kernels' scalar bf16 store truncates (max-pool values are bf16 already: only the average-pool backward rounds)",
   "bf16 storage, avgpool_bwd_kernel",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-avgpool_bf16]"])

# kernels_optim.hip
_m("lars_denominator_no_wd", "kernels_optim.hip",
   "tr = trust_coef * wn / (gn + wd * wn);",
   "tr = trust_coef * wn / gn;",
   "the LARS trust ratio's denominator drops wd * |w|",
   "weight tensors, wd > 0",
   ["tests/test_gpu_optim.py::test_operator_per_element_at_resnet50_geometry[lars-5e-05]"])
_m("lars_wd_on_gamma_beta", "kernels_optim.hip",
   "else wdt = 0.f;",
   "else wdt = wd;",
   "LARS keeps weight decay on BN gamma / beta and the FC bias",
   "non-weight tensors, wd > 0",
   ["tests/test_gpu_optim.py::test_operator_per_element_at_resnet50_geometry[lars-5e-05]"])
_m("optim_scalar_tail_no_momentum", "kernels_optim.hip",
   "opt_elem<KIND>(w, q, b, s, wdt, lr, mu, skip, bad);",
   "opt_elem<KIND>(w, q, b, s, wdt, lr, 0.f, skip, bad);",
   "the scalar tail behind the float4 body of a chunk runs with momentum 0: the last len % 4 elements of a tensor",
   "tensors whose length is no multiple of 4",
   ["tests/test_gpu_optim.py::test_operator_scalar_tail[sgd]", "tests/test_gpu_optim.py::test_operator_scalar_tail[lars]"])

_m("ema_unfused", "kernels_optim.hip",
   "    const float r = w < 0.5f ? fmaf(w, d, e) : fmaf(-omw, d, pv);",
   "    float r;\n    {\n#pragma clang fp contract(off)\n        const float t = w < 0.5f ? w * d : -omw * d;\n        r = w < 0.5f ? t + e : t + pv;\n    }",
   "ema_elem rounds the product and the sum one after the other instead of one fma: 47 to 65 of about 1024 elements at w = 0.1",
   "every element of ema_update_kernel",
   [EMA + "test_ema_kernel_is_the_model[vector-w=0.1]", EMA + "test_ema_kernel_is_the_model[element-wise-w=0.8]"])
_m("ema_branch_le_half", "kernels_optim.hip",
   "    const float r = w < 0.5f ? fmaf(w, d, e)",
   "    const float r = w <= 0.5f ? fmaf(w, d, e)",
   "ema_elem takes the branch around e at w = 0.5 (torch.lerp takes the one around p there): about 40 of 1024 elements",
   "w == 0.5",
   # CPU pre-check (emaref.other_branch32 on _pair's inputs): 39 / 41 / 42 elements at n = 1023 / 1024 / 1025
   [EMA + "test_ema_kernel_is_the_model[vector-w=0.5]"])
_m("ema_no_finite_guard", "kernels_optim.hip",
   "    return fin(r) ? r : e;",
   "    return r;",
   "ema_elem stores a result that is not finite instead of keeping e",
   "elements whose p, e or difference is not finite",
   [EMA + "test_ema_kernel_keeps_elements_that_would_not_be_finite[vector-p]"])
_m("ema_tail_unfused", "kernels_optim.hip",
   "        if (i < n) ema[i] = ema_elem(ema[i], p[i], w, omw);",
   "        if (i < n) {\n#pragma clang fp contract(off)\n            const float e0 = ema[i], p0 = p[i], d0 = p0 - e0, t0 = w < 0.5f ? w * d0 : -omw * d0;\n"
   "            const float r0 = w < 0.5f ? t0 + e0 : t0 + p0;\n            ema[i] = fin(r0) ? r0 : e0;\n        }",
   "the n % 4 elements behind the last float4 of ema_update_kernel<4> are updated without the fma (1 to 3 elements of an arena)",
   "the vector tail line of ema_update_kernel",
   # CPU pre-check: _pair's inputs separate none of these elements at n <= 5 and few beyond; emaref.separating_pair separates all
   [EMA + "test_ema_tails_and_partial_turns_on_inputs_that_separate_the_alternatives[vector-w=0.1]",
    EMA + "test_ema_tails_and_partial_turns_on_inputs_that_separate_the_alternatives[vector-w=0.8]"])
_m("exchange_tail_one_way", "kernels_optim.hip",
   "if (i < n) { const uint32_t x = a[i], y = b[i]; a[i] = y; b[i] = x; }",
   "if (i < n) { const uint32_t x = a[i], y = b[i]; a[i] = y; b[i] = y; }",
   "the n % 4 words behind the last uint4 of exchange_kernel<4> go from b to a only: b keeps its words",
   "the vector tail line of exchange_kernel",
   [EMA + "test_exchange_kernel_swaps_words[vector]"])
_m("exchange_turn_item2_one_way", "kernels_optim.hip",
   "                av[i] = y[k]; bv[i] = x[k];",
   "                av[i] = y[k]; bv[i] = k == 2 ? y[k] : x[k];",
   "the third of the four items a thread moves in a whole turn of exchange_kernel goes from b to a only",
   "whole (unrolled) turns of exchange_kernel",
   [EMA + "test_exchange_kernel_swaps_words[vector]", EMA + "test_exchange_kernel_swaps_words[element-wise]"])
_m("accum_first_adds_zero", "kernels_optim.hip",
   "    if (MODE == MID_ACC_FIRST) return q;",
   "    if (MODE == MID_ACC_FIRST) return __float_as_uint(__uint_as_float(q) + 0.f);",
   "grad_accum FIRST passes the gradient through an addition of 0: -0 becomes +0 (and a signalling NaN quiet)",
   "grad_accum_kernel<first>, words that arithmetic changes",
   [ACC + "test_kernel_is_the_model[first-vector]", ACC + "test_kernel_propagates_what_is_not_finite[first-element-wise]"])
_m("accum_fold_rounded_once", "kernels_optim.hip",
   "    const float scaled = sum * scale;",
   "    const float scaled = (float)(((double)__uint_as_float(a) + (double)__uint_as_float(q)) * (double)scale);",
   "grad_accum FOLD evaluates (acc + g) scale in double and rounds once: about a quarter of the elements at scale 1 / 3",
   "grad_accum_kernel<fold>, every element",
   [ACC + "test_fold_rounds_the_sum_and_the_product_separately", ACC + "test_kernel_is_the_model[fold-element-wise]"])
_m("accum_partial_turn_reads_g_twice", "kernels_optim.hip",
   "                out[it] = acc_item<MODE>(x, y, scale);",
   "                out[it] = acc_item<MODE>(y, y, scale);",
   "the partial turn of grad_accum_kernel takes the gradient for the accumulator's value as well (g + g); whole turns and the tail do not",
   "the partial-turn branch of grad_accum_kernel (ADD and FOLD)",
   [ACC + "test_tails_and_partial_turns_on_inputs_that_separate_the_alternatives[add-vector]",
    ACC + "test_tails_and_partial_turns_on_inputs_that_separate_the_alternatives[fold-element-wise]"])
_m("accum_tail_fold_rounded_once", "kernels_optim.hip",
   "            (MODE == MID_ACC_FOLD ? g : acc)[i] = acc_word<MODE>(x, y, scale);",
   "            (MODE == MID_ACC_FOLD ? g : acc)[i] = MODE == MID_ACC_FOLD\n"
   "                ? __float_as_uint((float)(((double)__uint_as_float(x) + (double)__uint_as_float(y)) * (double)scale)) : acc_word<MODE>(x, y, scale);",
   "the n % 4 elements behind the last uint4 of grad_accum_kernel<4, fold> are rounded once, through double",
   "the vector tail line of grad_accum_kernel<fold>",
   [ACC + "test_tails_and_partial_turns_on_inputs_that_separate_the_alternatives[fold-vector]"])

# kernels_input.hip
_m("mix_pair_fma", "kernels_input.hip",
   "    const float na = la + mb, nb = lb + ma;",
   "    const float na = fmaf(lam, a, mb), nb = fmaf(lam, b, ma);",
   "mix_pair contracts lam a + (mu b) into one fma: one rounding fewer in both results",
   "every element of mixup_kernel",
   [MIX + "test_mixup[2-8-0.3]", MIX + "test_mixup[2-7-0.3]"])
_m("mixup_elem_partner_weight", "kernels_input.hip",
   "            mix_pair(va, vb, lam, mu);\n            a[e] = va; b[e] = vb;",
   "            mix_pair(va, vb, lam, lam);\n            a[e] = va; b[e] = vb;",
   "the element-wise branch of mixup_kernel weighs the partner with lam instead of 1 - lam",
   "the element-wise branch of mixup_kernel",
   [MIX + "test_mixup[2-7-0.3]", MIX + "test_mixup_on_an_unaligned_batch"])
_m("mixup_second_turn_keeps", "kernels_input.hip",
   "i < items; i += step) {\n        if (i < quads) {",
   "i < items; i += step) {\n        lam = i >= step ? 1.f : lam; mu = i >= step ? 0.f : mu;\n        if (i < quads) {",
   "work items a thread of mixup_kernel reaches after its first (i >= step) are mixed with lam = 1, mu = 0: they keep their values",
   "the second and later grid-stride turns of mixup_kernel",
   [MIX + "test_mixup_takes_a_second_grid_stride_turn[vec]", MIX + "test_mixup_takes_a_second_grid_stride_turn[elem]"])
_m("cutmix_groups_second_lane_turn_keep_b", "kernels_input.hip",
   "for (int q = lane; q < nq; q += 64) { const uint4 t = qa[q]; qa[q] = qb[q]; qb[q] = t; }",
   "for (int q = lane; q < nq; q += 64) { const uint4 t = qa[q], o = qb[q]; qa[q] = o; qb[q] = q >= 64 ? o : t; }",
   "the 16-byte groups q >= 64 of a row segment (a lane's second turn) go from b to a only: b keeps its words",
   "cutmix_kernel, 16-byte path, boxes more than 64 groups wide",
   [MIX + "test_cutmix_wide_and_tall_boxes[vec-x3_inner]", MIX + "test_cutmix_wide_and_tall_boxes[vec-whole]"])
_m("cutmix_elems_from_64_keep_b", "kernels_input.hip",
   "for (int e = 64 + lane; e < w; e += 64) { const uint32_t t = pa[e]; pa[e] = pb[e]; pb[e] = t; }",
   "for (int e = 64 + lane; e < w; e += 64) { const uint32_t o = pb[e]; pa[e] = o; pb[e] = o; }",
   "the elements e >= 64 of a row segment on the element-wise path go from b to a only: b keeps its words",
   "cutmix_kernel, element-wise path, boxes more than 64 columns wide",
   [MIX + "test_cutmix_wide_and_tall_boxes[elem-x3_inner]"])
_m("cutmix_second_sweep_keep_b", "kernels_input.hip",
   "        if (lane < head) { const uint32_t t = pa[lane]; pa[lane] = pb[lane]; pb[lane] = t; }\n"
   "        if (!vec) for (int e = 64 + lane; e < w; e += 64) { const uint32_t t = pa[e]; pa[e] = pb[e]; pb[e] = t; }\n"
   "        else {\n"
   "            uint4 *qa = (uint4 *)(pa + head), *qb = (uint4 *)(pb + head);\n"
   "            for (int q = lane; q < nq; q += 64) { const uint4 t = qa[q]; qa[q] = qb[q]; qb[q] = t; }\n",
   "        const bool late = sgm >= (int)gridDim.x * waves;\n"
   "        if (lane < head) { const uint32_t t = pa[lane], o = pb[lane]; pa[lane] = o; pb[lane] = late ? o : t; }\n"
   "        if (!vec) for (int e = 64 + lane; e < w; e += 64) { const uint32_t t = pa[e], o = pb[e]; pa[e] = o; pb[e] = late ? o : t; }\n"
   "        else {\n"
   "            uint4 *qa = (uint4 *)(pa + head), *qb = (uint4 *)(pb + head);\n"
   "            for (int q = lane; q < nq; q += 64) { const uint4 t = qa[q], o = qb[q]; qa[q] = o; qb[q] = late ? o : t; }\n",
   "row segments a wave of cutmix_kernel reaches after its first (sgm >= gridDim.x * waves) go from b to a only, on both paths",
   "the second sweep of the segment loop of cutmix_kernel (3 h > 512 segments)",
   [MIX + "test_cutmix_wide_and_tall_boxes[elem-from_1_1]", MIX + "test_cutmix_wide_and_tall_boxes[vec-from_1_1]"])
_m("cutmix_tail_behind_groups_keep_b", "kernels_input.hip",
   "            if (e < w) { const uint32_t t = pa[e]; pa[e] = pb[e]; pb[e] = t; }",
   "            if (e < w) { const uint32_t o = pb[e]; pa[e] = o; pb[e] = o; }",
   "the elements behind the last 16-byte group of a row segment go from b to a only",
   "cutmix_kernel, 16-byte path, the one-lane-each tail",
   # D = 30, columns 3 .. 28: rows whose segment starts 1 word past a 16-byte boundary have 3 + 5 x 4 + 3 elements
   [MIX + "test_cutmix[2-30-x3_w26]"])
_m("decode_r_plane_b_mean", "kernels_input.hip",
   "{123.68, 116.78, 103.94}; // subtracted from source byte 0",
   "{123.68, 116.78, 123.68}; // subtracted from source byte 0",
   "the decode subtracts the B mean from the R plane",
   "one of three planes",
   ["tests/test_gpu_input_u8.py::test_decode_sweep[37-30-1]"])
_m("resample_row_weight", "kernels_input.hip",
   "(double)(top * (256 - wy) + bot * wy)",
   "(double)(top * (255 - wy) + bot * wy)",
   "the resample blends the upper source row with weight 255 - wy",
   "every element",
   ["tests/test_gpu_input_rrc.py::test_resample_sweep[37-30-1]"])
_m("resample_tail_no_row_weight", "kernels_input.hip",
   "out_n[(2 - p) * plane + (size_t)(h0 + r) * D + ox] = rs_value(L0, L1, x0, x1, wx, wy, p);",
   "out_n[(2 - p) * plane + (size_t)(h0 + r) * D + ox] = rs_value(L0, L1, x0, x1, wx, 0, p);",
   "the scalar tail columns of the resample (dim_out % 4 of them) ignore the vertical weight",
   "the last dim_out % 4 columns of a row",
   ["tests/test_gpu_input_rrc.py::test_resample_sweep[37-30-1]"])

# resample_aa_u8_kernel.  mi_aa.h takes no mutant (the one header slot is mi_common.hpp's, and loader.c compiles the same text): a fault
# in the table's arithmetic is planted where the kernel stores the table.  e[0] (first tap) and e[1] (tap count) are an address and a
# bound and are never touched; the coefficients e[2 ...] are values.  The cases are (dim_in, virt, dim_out, window) of AA + CASES;
# tests/test_input_aa.py restates every entry in the numpy model and holds, without a GPU, that each killer's own inputs separate it.
_m("aa_col_truncates", "kernels_input.hip",
   "int s0 = 1 << (MI_AA_BITS - 1), s1 = s0, s2 = s0;",
   "int s0 = 0, s1 = s0, s2 = s0;",
   "the column pass of the antialiased resize starts its three sums at 0 instead of 2^21: it truncates where Pillow rounds",
   "resample_aa_u8_kernel, the column pass, every element",
   [AA + "test_sweep[9-4-4-0]"])
_m("aa_row_truncates", "kernels_input.hip",
   "for (int t = 0; t < 12; t++) acc[t] = 1 << (MI_AA_BITS - 1);",
   "for (int t = 0; t < 12; t++) acc[t] = 0;",
   "the row pass starts the twelve sums of a quad at 0 instead of 2^21: every column but the last dim_out % 4",
   "resample_aa_u8_kernel, the row pass over quads",
   [AA + "test_sweep[9-4-4-0]"])
_m("aa_tail_truncates", "kernels_input.hip",
   "int s = 1 << (MI_AA_BITS - 1);",
   "int s = 0;",
   "the scalar tail of the row pass starts its sum at 0 instead of 2^21: the last dim_out % 4 columns",
   "resample_aa_u8_kernel, the row pass over the last dim_out % 4 columns",
   [AA + "test_sweep[33-7-7-0]"])
_m("aa_value_r_plane_b_mean", "kernels_input.hip",
   "103.94}; // as g_decode_table\n    return (float)((double)(float)b - mean_of_src[p]);",
   "123.68}; // as g_decode_table\n    return (float)((double)(float)b - mean_of_src[p]);",
   "aa_value's own mean table takes the B mean for source position 2: the R plane of every image",
   "aa_value, one of three planes",
   [AA + "test_sweep[8-1-1-0]"])
_m("aa_scalar_store_lane3", "kernels_input.hip",
   "for (int j = 0; j < 4; j++) o[d3 * plane + j] = v[2 - d3][j];",
   "for (int j = 0; j < 4; j++) o[d3 * plane + j] = v[2 - d3][j] + (j == 3 ? 0.0625f : 0.f);",
   "the element-wise store of a quad (vec == 0) adds 2^-4 to its fourth value: every fourth column where out is off a 16-byte boundary or "
   "dim_out % 4 != 0",
   "resample_aa_u8_kernel, the row pass over quads, the element-wise stores",
   [AA + "test_sweep[33-7-7-0]", AA + "test_into_an_output_one_float_off_alignment[32-8-8-0]"])
_m("aa_ctab_first_coeff_low", "kernels_input.hip",
   "e[0] = lo - xa; e[1] = min(taps, ks);",
   "e[0] = lo - xa; e[1] = min(taps, ks); e[2] -= (e[1] > 1);",
   "the first coefficient of every column-table entry with more than one tap is one unit of 2^-22 low: only outputs whose column sum lies "
   "within one byte value of a rounding boundary change, so only tie-prone ratios see it",
   "resample_aa_u8_kernel, the column table as stored",
   # CPU pre-check (tests/test_input_aa.py), elements of the three whole+corner images that change: 340 / 357 / 75 of 1728 each at
   # 16 -> 24, 250 / 222 / 133 of 8112 at 64 -> 58; none in the whole images at 9 -> 4 and 33 -> 7
   [AA + "test_sweep[16-24-24-0]", AA + "test_sweep[64-58-52-3]"])
_m("aa_rtab_last_coeff_high", "kernels_input.hip",
   "e[0] = lo - ya; e[1] = min(taps, ks);",
   "e[0] = lo - ya; e[1] = min(taps, ks); e[2 + e[1] - 1] += (e[1] > 1);",
   "the last coefficient of every row-table entry with more than one tap is one unit of 2^-22 high (e[1] >= 1 is the count of coefficients "
   "the entry holds: the store stays inside it): as aa_ctab_first_coeff_low, vertical",
   "resample_aa_u8_kernel, the row table as stored",
   # CPU pre-check: 86 / 86 / 21 elements at 16 -> 24, 85 / 94 / 50 at 64 -> 58
   [AA + "test_sweep[16-24-24-0]", AA + "test_sweep[64-58-52-3]"])
_m("aa_col_blue_first_tap_zero", "kernels_input.hip",
   "s0 += L[3 * j] * k;",
   "s0 += L[3 * j] * (j == 0 ? 0 : k);",
   "the column pass multiplies the first tap of source channel 0 by 0: the B plane",
   "resample_aa_u8_kernel, the column pass, one source channel",
   [AA + "test_sweep[9-4-4-0]"])
_m("aa_row_second_turn_plus_one", "kernels_input.hip",
   "v[p][j] = aa_value(min(acc[3 * j + p] >> MI_AA_BITS, 255), p);",
   "v[p][j] = aa_value(min(acc[3 * j + p] >> MI_AA_BITS, 255) + (i >= AA_THREADS ? 1 : 0), p);",
   "quads a thread of the row pass reaches after its first (i >= 256) come out one byte value high: rows and quads past item 255 of a "
   "workgroup",
   "the second and later grid-stride turns of the row pass (R (dim_out / 4) > 256: dim_out >= 68)",
   # 16 x 17 = 272 items: the last 16 quads of row 15 of every full workgroup; 15 x 25 = 375 items under R = 15
   [AA + "test_sweep[100-68-68-0]", AA + "test_sweep[294-100-100-0]"])
_m("aa_ctab_past_256_first_tap_zero", "kernels_input.hip",
   "e[0] = lo - xa; e[1] = min(taps, ks);",
   "e[0] = lo - xa; e[1] = min(taps, ks); e[2] = i >= AA_THREADS ? 0 : e[2];",
   "column-table entries a thread fills after its first (i >= 256) get first coefficient 0: window columns 256 and up, or columns "
   "0 .. dim_out - 257 of a flipped image",
   "the second grid-stride turn of the column-table fill (dim_out > 256)",
   [AA + "test_sweep[300-260-260-0]"])
_m("aa_stage_pieces_past_64_zero", "kernels_input.hip",
   "*(uint4 *)(raw + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);",
   "*(uint4 *)(raw + ((size_t)r * CH + c) * 16) = c >= 64 ? make_uint4(0u, 0u, 0u, 0u) : load16_in_batch(src, a, total_bytes);",
   "the 16-byte pieces of a source row that a lane stages after its first (c >= 64) are stored as zeros: source bytes from 1024 on, "
   "counted from the row span's start rounded down to 16",
   "the second lane turn of the staging loop (boxes of 337 columns and more)",
   # no case of the sweep is that wide; the image one pixel under the LDS limit is (468 columns, 89 pieces, R = 1).  CPU pre-check: 569 of
   # its 1728 elements change
   [AA + "test_refuses_an_image_too_wide_for_lds"])
_m("aa_rtab_row9_first_tap_zero", "kernels_input.hip",
   "e[0] = lo - ya; e[1] = min(taps, ks);",
   "e[0] = lo - ya; e[1] = min(taps, ks); e[2] = i == 9 ? 0 : e[2];",
   "row-table entry 9 of every workgroup gets first coefficient 0: window rows = 9 mod R where a workgroup has at least 10 rows, none "
   "where R <= 9.  The pair of killers says that the row tables are per workgroup: 16 -> 24 (R = 16) fails in row 9 (and no other); "
   "200 -> 24 (R = 9, workgroups of 9, 9 and 6 rows) must NOT show the fault in any row and alone does not kill it -- it passes, and "
   "would fail if the table were indexed by the window row",
   "resample_aa_u8_kernel, the row table as stored, one entry of a workgroup",
   # the R = 9 case stands first: the child stops at its first failure (-x), so this order is the one in which both run
   [AA + "test_sweep[200-24-24-0]", AA + "test_sweep[16-24-24-0]"])

# kernels_loss.hip
_m("loss_u_over_l_minus_1", "kernels_loss.hip",
   "const float u = eps / (float)L, tc",
   "const float u = eps / (float)(L - 1), tc",
   "the smoothing mass per class is eps / (L - 1)",
   "eps > 0",
   ["tests/test_gpu_loss_head.py::test_loss_head[shape1-0.1]"])
_m("loss_rank_tie_strict", "kernels_loss.hip",
   "p_ >= pc) ? 1 : 0;",
   "p_ > pc) ? 1 : 0;",
   "the rank counts p_j > p_c: ties no longer count against the label",
   "rows with ties",
   ["tests/test_gpu_loss_head.py::test_loss_head[shape1-0.0]"])
_m("loss_long_row_float_sum", "kernels_loss.hip",
   "szd += (double)z;",
   "szd = (double)(float)((float)szd + z);",
   "rows longer than LOSS_REG_COLS add z per lane in float instead of double",
   "loss_head_kernel<mem> (L > 1024)",
   ["tests/test_gpu_loss_head.py::test_long_row_sums_z_in_double"])
_m("loss_mix_wb_as_difference", "kernels_loss.hip",
   "wb = MIX ? loss_mul_rn(1.f - eps, 1.f - lam) : 0.f;",
   "wb = MIX ? loss_add_rn(1.f - eps, -wa) : 0.f;",
   "the two-label head forms the second weight as (1 - eps) - wa instead of the product (1 - eps)(1 - lam): the neighbouring float at some lam",
   "loss_head_kernel<*, MIX>, t_b of every row",
   # CPU pre-check (tests/test_mix_model.py): the same float32 at lam = 0.3 with eps 0 and 0.1 -- test_loss_head_mix cannot see it --, the
   # neighbouring one at lam = 0.7, eps = 0.1
   [MIX + "test_second_weight_is_one_rounded_product"])
_m("loss_mix_drops_wb_zb", "kernels_loss.hip",
   "logf(s) - wa * zc - wb * zb - u * sz",
   "logf(s) - wa * zc - u * sz",
   "the two-label row loss lacks the second label's term wb z_b",
   "loss_head_kernel<*, MIX>, row_loss with wb > 0",
   [MIX + "test_loss_head_mix[shape1-0.3-0.0]"])
_m("loss_mix_target_sum_reassociated", "kernels_loss.hip",
   "loss_add_rn(loss_add_rn(valid && (j_) == c ? wa : 0.f, valid_b && (j_) == cb ? wb : 0.f), u)",
   "loss_add_rn(valid && (j_) == c ? wa : 0.f, loss_add_rn(valid_b && (j_) == cb ? wb : 0.f, u))",
   "the two-label target is summed as wa + (wb + u): another float32 where both labels are one class and the roundings fall that way",
   "loss_head_kernel<*, MIX>, rows with a == b",
   # CPU pre-check (tests/test_mix_model.py): of lossref.SHAPES at lam 0.3, eps 0.1 only L = 65 separates (all 4 rows); a != b never does
   [MIX + "test_loss_head_mix[shape3-0.3-0.1]"])
_m("loss_reduce_topk_strict", "kernels_loss.hip",
   "wk += row_rank[r] >= topk ? 1 : 0;",
   "wk += row_rank[r] > topk ? 1 : 0;",
   "the batch totals count a row as top-k wrong only where rank > k: rows whose rank is exactly k are missed",
   "loss_reduce_kernel, rows with rank == topk",
   [LOSS + "test_batch_totals_past_64_rows_and_at_the_topk_threshold[5-0.0]", MIX + "test_batch_totals_past_64_rows_and_at_the_topk_threshold[1-0.1]"])
_m("loss_reduce_rows_past_64_zero", "kernels_loss.hip",
   "        sum += (double)row_loss[r];\n        w1 += row_rank[r] >= 1 ? 1 : 0;\n        wk += row_rank[r] >= topk ? 1 : 0;",
   "        sum += (r >= 64 ? 0.0 : 1.0) * (double)row_loss[r];\n        w1 += (r >= 64 ? 0 : 1) * (row_rank[r] >= 1 ? 1 : 0);\n"
   "        wk += (r >= 64 ? 0 : 1) * (row_rank[r] >= topk ? 1 : 0);",
   "the batch totals multiply the rows a lane reaches after its first (r >= 64) by 0: the loss sum and both counts lack them",
   "loss_reduce_kernel, the second and later passes of the lanes (N > 64)",
   [LOSS + "test_batch_totals_past_64_rows_and_at_the_topk_threshold[10-0.0]"])
_m("loss_reduce_float_lane_sum", "kernels_loss.hip",
   "sum += (double)row_loss[r];",
   "sum = (double)(float)((float)sum + row_loss[r]);",
   "the lanes of loss_reduce_kernel add their rows in float: loss_sum is about 5e-9 off (relative) at two or three rows per lane",
   "loss_reduce_kernel, lanes with more than one row (N > 64)",
   [LOSS + "test_batch_totals_past_64_rows_and_at_the_topk_threshold[10-0.1]"])

# ---------------------------------------------------------------------------------------------------------------------------
# The loop turns of the first-generation element-wise kernels ("Suite sensitivity", "Loop turns of the
# first-generation element-wise kernels"): one entry per whole turn, remainder, inter-wave merge, straddle, second grid-stride turn and second lane turn.  The reach
# of every killer is worked out from the launchers' formulas in the "reach" table there; tests/test_loop_turns_model.py holds, without a
# GPU, that the killers' own inputs separate the restated fault.
LT = RAG + "test_bn_loop_turns"
OPT = "tests/test_gpu_optim.py::"
U8 = "tests/test_gpu_input_u8.py::"
RRC = "tests/test_gpu_input_rrc.py::"

# kernels_bn.hip
_m("bn_stats_turn_unit3_m2_zero", "kernels_bn.hip",
   "                    m2 += (a * a + b * b) + (cc * cc + d * d);",
   "                    m2 += (u == 3 ? 0.f : 1.f) * ((a * a + b * b) + (cc * cc + d * d));",
   "the whole turn of bn_stats_kernel (four units in flight, V > 1) multiplies the squared deviations of its fourth unit by 0: the variance "
   "of every channel whose block has 1024 units or more",
   "bn_stats_kernel, the four-in-flight loop, V > 1 (cnt P / V >= 1024)",
   # of the nets' planes only the 112^2 stem reaches it (8 splits of one image, 3136 float4 units); test_bn_loop_turns has the small
   # shapes with a whole turn and a remainder (N = 1, C = 64, H = 66: 1089 units)
   [RAG + "test_bn_fwd_ragged[r50_N8-f32_C64_H112]"])
_m("bn_stats_turn_scalar_fourth_deviation", "kernels_bn.hip",
   "wel_add_batch(w, 4.f, bm, (a * a + b * b) + (cc * cc + d * d));",
   "wel_add_batch(w, 4.f, bm, (a * a + b * b) + (cc * cc + 0.f * d * d));",
   "the whole turn of bn_stats_kernel<V = 1> drops the fourth squared deviation of a batch of four",
   "bn_stats_kernel, the four-in-flight loop, V == 1 (planes of 49: cnt >= 21)",
   # C = 2048: one split; N = 21 x 49 = 1029 scalar units: one whole turn, 5 units of remainder
   [LT + "[f32_C2048_H7_N21]"])
_m("bn_stats_remainder_add4_fourth_deviation", "kernels_bn.hip",
   "t.m2 = (da * da + db * db) + (dc * dc + dd * dd);",
   "t.m2 = (da * da + db * db) + (dc * dc + 0.f * dd * dd);",
   "wel_add4 (called by the remainder loop of bn_stats_kernel only) drops the fourth squared deviation",
   "bn_stats_kernel, the remainder loop, V > 1",
   [RAG + "test_bn_fwd_ragged[c1s_N4-f32_C64_H8]"])
_m("bn_stats_remainder_add1_half_mean", "kernels_bn.hip",
   "Wel t; t.n = 1.f; t.mean = a; t.m2 = 0.f;",
   "Wel t; t.n = 1.f; t.mean = 0.5f * a; t.m2 = 0.f;",
   "wel_add1 (called by the remainder loop of bn_stats_kernel<V = 1> only) enters every value at half its size",
   "bn_stats_kernel, the remainder loop, V == 1",
   [RAG + "test_bn_fwd_ragged[r50_N8-f32_C512_H7]"])
_m("bn_stats_interwave_wave3_count_zero", "kernels_bn.hip",
   "for (int i = 1; i < (int)(blockDim.x >> 6); i++) r = wel_merge(r, sh[i]);",
   "for (int i = 1; i < (int)(blockDim.x >> 6); i++) { Wel t_ = sh[i]; t_.n = i == 3 ? 0.f : t_.n; r = wel_merge(r, t_); }",
   "the inter-wave merge of bn_stats_kernel takes the fourth wave's partial with n = 0: its mean is ignored and the total count is short",
   "bn_stats_kernel, the merge of the four waves (the fourth wave holds data from 193 units on)",
   # c1s_N4-f32_C64_H8 has 16 units per block: wave 3 holds n = 0 there anyway.  r50_N8-f32_C64_H56: 784 units
   [RAG + "test_bn_fwd_ragged[r50_N8-f32_C64_H56]"])
_m("bn_parts_merge_turn_item7_m2_zero", "kernels_bn.hip",
   "for (int u = 0; u < 8; u++) w = wel_merge(w, b[u]);",
   "for (int u = 0; u < 8; u++) { Wel t_ = b[u]; t_.m2 = u == 7 ? 0.f : t_.m2; w = wel_merge(w, t_); }",
   "the eight-in-flight loop of bn_parts_merge_kernel takes the eighth partial's M2 as 0",
   "bn_parts_merge_kernel, whole turns (more than 28 partials per chunk)",
   # plan (64, 128, 52, 52, 1, 1, 0): 13 column tiles x 4 = 52 partials, one chunk: one whole turn per sub-group, then 5 partials
   [RAG + "test_conv_bn_fwd_ragged[r50_N8-bf16_C1024_H14_K256_k1_s1]"])
_m("bn_parts_merge_remainder_m2_zero", "kernels_bn.hip",
   "Wel b = {parts[o], parts[plane + o], parts[2 * plane + o]};",
   "Wel b = {parts[o], parts[plane + o], 0.f * parts[2 * plane + o]};",
   "the remainder loop of bn_parts_merge_kernel takes every partial's M2 as 0",
   "bn_parts_merge_kernel, the remainder loop",
   [RAG + "test_conv_bn_fwd_ragged[c1s_N4-f32_C64_H8_K64_k1_s1]"])
_m("bn_parts_merge_subgroup3_dropped", "kernels_bn.hip",
   "for (int i = 1; i < 4; i++) r = wel_merge(r, sh[i][cx]);",
   "for (int i = 1; i < 4; i++) { Wel t_ = sh[i][cx]; if (i == 3) { t_.n = 0.f; t_.mean = 0.f; t_.m2 = 0.f; } r = wel_merge(r, t_); }",
   "the merge of the four sub-groups of bn_parts_merge_kernel leaves the fourth out: a quarter of the partials",
   "bn_parts_merge_kernel, the merge of the sub-groups",
   [RAG + "test_conv_bn_fwd_ragged[c1s_N4-f32_C64_H8_K64_k1_s1]"])
_m("bn_finalize_lanes_from_16_m2_zero", "kernels_bn.hip",
   "if (lane < nsplit) { w.n = p[lane * 3]; w.mean = p[lane * 3 + 1]; w.m2 = p[lane * 3 + 2]; }",
   "if (lane < nsplit) { w.n = p[lane * 3]; w.mean = p[lane * 3 + 1]; w.m2 = (lane >= 16 ? 0.f : 1.f) * p[lane * 3 + 2]; }",
   "bn_finalize_kernel takes the M2 of the partials in lanes 16 and up as 0",
   "bn_finalize_kernel, lanes 16 .. 63 (more than 16 splits: N > 16 and C <= 120)",
   # N = 33, C = 64: 32 splits, the first with two images
   [LT + "[f32_C64_H4_N33]"])
_m("bn_bwd_finalize_lanes_from_16_s2_zero", "kernels_bn.hip",
   "if (lane < nsplit) { s1 = p[lane * 3]; s2 = p[lane * 3 + 1]; }",
   "if (lane < nsplit) { s1 = p[lane * 3]; s2 = (lane >= 16 ? 0.f : 1.f) * p[lane * 3 + 1]; }",
   "bn_bwd_finalize_kernel takes the second sum of the partials in lanes 16 and up as 0: dgamma, and dx through it",
   "bn_bwd_finalize_kernel, lanes 16 .. 63",
   # N = 33, C = 64: 32 splits of bn_bwd_reduce_kernel's own grid (at most 8 at N = 8: r50_N8-f32_C64_H56_mode1 passes under this fault).
   # Of the suite as it was, the fused dgrad of r50_N8-bf16_C64_H56_K256_k1_s1 killed it: 784 partials, 64 chunks
   [RAG + "test_bn_bwd_loop_turns[f32_C64_H4_N33_mode0]", RAG + "test_dgrad_bn_bwd_ragged[r50_N8-bf16_C64_H56_K256_k1_s1]"])
_m("bn_apply_straddle_sd", "kernels_bn.hip",
   "sd1 = sqrtf(vars[c1] + eps); g1 = gamma[c1]; b1 = beta[c1];\n        }",
   "sd1 = sd0; g1 = gamma[c1]; b1 = beta[c1];\n        }",
   "in a vector that straddles two channel planes the second channel's elements are divided by the first channel's standard deviation",
   "bn_apply_kernel, the straddling vectors of 7 x 7 planes (STR)",
   [RAG + "test_bn_fwd_ragged[r50_N8-f32_C512_H7]"])
_m("bn_apply_norm_out_after_relu", "kernels_bn.hip",
   "if (norm_out) VecIO<float, V>::store(norm_out + e, nv);",
   "if (norm_out) VecIO<float, V>::store(norm_out + e, v);",
   "bn_apply_kernel stores the value after the ReLU (and the residual) as norm_out, the BN output the FULL store policy keeps",
   "bn_apply_kernel, the xhat_out / norm_out stores (the trainer's FULL store policy; no operator passes them)",
   [OPS + "test_full_store_policy_tensors_per_element"])
_m("bn_apply_cl_short_piece_last_residual_zero", "kernels_bn.hip",
   "r[q] = (residual && q < nv) ? mi_bf2f(residual[e + q]) : 0.f;",
   "r[q] = (residual && q < nv) ? (q == nv - 1 ? 0.f : 1.f) * mi_bf2f(residual[e + q]) : 0.f;",
   "bn_apply_cl_kernel reads the residual of the last element of a plane's short last piece (P % 8 != 0) as 0",
   "bn_apply_cl_kernel, the nv < 8 branch with a residual",
   # 14 x 14 = 196 = 24 x 8 + 4; "cl par add_relu" is the expansion BN's form
   [RAG + "test_bn_fwd_ragged[r50_N8-bf16_C1024_H14]"])
_m("bn_apply_cl_tile_odd_pixel_takes_even", "kernels_bn.hip",
   "tile[(part * 8 + 2 * q + 1) * 72 + cc] = (bf16_t)(o[q] >> 16);",
   "tile[(part * 8 + 2 * q + 1) * 72 + cc] = (bf16_t)(o[q] & 0xffffu);",
   "the tile fill of bn_apply_cl_kernel gives the odd pixel of a pair the even pixel's half-word: every second pixel of the channel-last copy",
   "bn_apply_cl_kernel, the LDS tile as filled",
   [RAG + "test_bn_fwd_ragged[c1s_N4-bf16_C64_H8]"])
_m("bn_bwd_reduce_turn_last_unit_s2", "kernels_bn.hip",
   "for (int q = 0; q < V; q++) gq[q] = one(xv[u][q], dv[u][q], mv[u][q]);",
   "for (int q = 0; q < V; q++) { const float keep_ = s2; gq[q] = one(xv[u][q], dv[u][q], mv[u][q]); s2 = u == U - 1 ? keep_ : s2; }",
   "the whole turn of bn_bwd_reduce_kernel leaves its last unit in flight out of the second sum: dgamma, and dx through it",
   "bn_bwd_reduce_kernel, the U-in-flight loop (U = 4: 1024 units; the external-mask modes U = 2: 512)",
   [RAG + "test_bn_bwd_ragged[r50_N8-f32_C64_H112_mode1]"])
_m("bn_bwd_reduce_remainder_last_element_s1", "kernels_bn.hip",
   "for (int q = 0; q < V; q++) gq[q] = one(xv[q], dv[q], mv[q]);",
   "for (int q = 0; q < V; q++) { const float keep_ = s1; gq[q] = one(xv[q], dv[q], mv[q]); s1 = q == V - 1 ? keep_ : s1; }",
   "the remainder loop of bn_bwd_reduce_kernel leaves the last element of every unit out of the first sum: dbeta, and dx through it",
   "bn_bwd_reduce_kernel, the remainder loop",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C256_H8_mode0]"])
_m("bn_bwd_reduce_remainder_gated_ungated", "kernels_bn.hip",
   "if (MASK == 3) VecIO<TA, V>::store(gated + o, gq);",
   "if (MASK == 3) VecIO<TA, V>::store(gated + o, dv);",
   "the remainder loop of bn_bwd_reduce_kernel<3> writes the ungated dy as the gated gradient",
   "bn_bwd_reduce_kernel, MASK == 3, the remainder loop's store",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C256_H8_mode3]"])
_m("bn_bwd_parts_merge_turn_item7_dropped", "kernels_bn.hip",
   "for (int u = 0; u < 8; u++) { a1 += u1[u]; a2 += u2[u]; }",
   "for (int u = 0; u < 8; u++) { a1 += u == 7 ? 0.f : u1[u]; a2 += u == 7 ? 0.f : u2[u]; }",
   "the eight-in-flight loop of bn_bwd_parts_merge_kernel leaves the eighth partial out of both sums",
   "bn_bwd_parts_merge_kernel, whole turns (more than 28 partials per chunk)",
   # plan (64, 128, 208, 208, 1, 1, 0): 13 column tiles x 4 = 52 partials, one chunk
   [RAG + "test_dgrad_bn_bwd_ragged[r50_N8-f32_C1024_H14_K256_k1_s1]"])
_m("bn_bwd_parts_merge_remainder_s2_zero", "kernels_bn.hip",
   "a1 += parts[o]; a2 += parts[plane + o];",
   "a1 += parts[o]; a2 += 0.f * parts[plane + o];",
   "the remainder loop of bn_bwd_parts_merge_kernel multiplies the second sum's partials by 0",
   "bn_bwd_parts_merge_kernel, the remainder loop",
   [RAG + "test_dgrad_bn_bwd_ragged[c1s_N4-bf16_C64_H8_K256_k1_s1]"])
_m("bn_bwd_parts_merge_no_eps", "kernels_bn.hip",
   "o[0] = s1; o[1] = s2 / sqrtf(vars[c] + eps);",
   "o[0] = s1; o[1] = s2 / sqrtf(vars[c]);",
   "bn_bwd_parts_merge_kernel divides the second sum by sqrtf(var) without eps: channels of small variance",
   "bn_bwd_parts_merge_kernel, the final division",
   # the fused-dgrad cases normalise N(0.3, 1.5^2) tensors: var = 2.25 against eps = 1e-7, and the fault survived both of them
   [RAG + "test_dgrad_bn_bwd_small_variance[f32]", RAG + "test_dgrad_bn_bwd_small_variance[bf16]"])
_m("bn_bwd_apply_straddle_k2", "kernels_bn.hip",
   "k11 = dbeta[c1] * inv_m; k21 = dgamma[c1] * inv_m; scale1 = g1 / sd1;",
   "k11 = dbeta[c1] * inv_m; k21 = k20; scale1 = g1 / sd1;",
   "in a vector that straddles two channel planes the second channel's dx takes the first channel's dgamma / M",
   "bn_bwd_apply_kernel, the straddling vectors of 7 x 7 planes (STR)",
   [RAG + "test_bn_bwd_ragged[r50_N8-f32_C2048_H7_mode0]"])
_m("bn_bwd_apply_gate_y_ge", "kernels_bn.hip",
   "if (MASK == 1) on = bn_y(xh, g, b) > 0.f;\n            if (MASK == 2) on = mv[q] > 0.f;",
   "if (MASK == 1) on = bn_y(xh, g, b) >= 0.f;\n            if (MASK == 2) on = mv[q] > 0.f;",
   "the recomputed gate of bn_bwd_apply_kernel is y >= 0: dx passes dy where y is exactly 0",
   "bn_bwd_apply_kernel, MASK == 1, elements with y == 0",
   [RAG + "test_bn_bwd_ragged[c1s_N4-f32_C64_H8_mode1]"])

# kernels_misc.hip
_m("maxpool_left_tap_never_wins", "kernels_misc.hip",
   "const float e = v[2 * j + c];",
   "const float e = (j == 0 && c == 0) ? -2048.f : v[2 * j + c];",
   "the left-neighbour tap of a cell of maxpool_fwd_3x3s2_kernel (the element in front of the 8-element vector) never wins: value and "
   "index of every fourth output whose maximum sits there",
   "maxpool_fwd_3x3s2_kernel, the has_left tap",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-maxpool_f32]"])
_m("maxpool_last_tap_never_wins", "kernels_misc.hip",
   "const float e = v[2 * j + c];",
   "const float e = (r == 1 && j == 3 && c == 2) ? -2048.f : v[2 * j + c];",
   "the last tap of a cell of maxpool_fwd_3x3s2_kernel (lower row, last of the nine columns) never wins",
   "maxpool_fwd_3x3s2_kernel, tap (r = 1, j = 3, c = 2)",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-maxpool_f32]"])
_m("maxpool_bwd_v11_first_writer", "kernels_misc.hip",
   "if (i11 == e11) v11 = d11;",
   "if (i11 == e11) v11 = (i00 == e11) ? d00 : d11;",
   "maxpool_bwd_3x3s2_kernel lets window (a, b) win over window (a + 1, b + 1) for the cell's last element",
   "maxpool_bwd_3x3s2_kernel, elements that are the arg-max of both diagonal windows",
   [RAG + "test_pools_softmax_fc_ragged[c1s_N4-maxpool_f32]"])
_m("maxpool_generic_last_of_equal_maxima", "kernels_misc.hip",
   "if (v > mv) { mv = v; mi = (int)pbase + ih * H + iw; }",
   "if (v >= mv) { mv = v; mi = (int)pbase + ih * H + iw; }",
   "the generic max-pool takes the last of equal maxima inside a window (the index stays in the window)",
   "maxpool_fwd_kernel (planes whose rows are no multiple of 8 elements)",
   [OPS + "test_maxpool[64-12-3]"])
_m("maxpool_generic_bwd_first_writer", "kernels_misc.hip",
   "if (idx[o] == (int)e) v = ldf<T>(dy + o);",
   "if (idx[o] == (int)e) v = v != 0.f ? v : ldf<T>(dy + o);",
   "the generic max-pool backward keeps the first window (with a dy other than 0) whose arg-max an element is, not the last",
   "maxpool_bwd_kernel (odd planes: every even plane takes maxpool_bwd_3x3s2_kernel)",
   [OPS + "test_maxpool[64-13-3]"])
_m("avgpool_second_lane_turn_zero", "kernels_misc.hip",
   "for (int i = lane; i < P; i += 64) s += ldf<T>(xp + i);",
   "for (int i = lane; i < P; i += 64) s += (i >= 64 ? 0.f : 1.f) * ldf<T>(xp + i);",
   "avgpool_fwd_kernel multiplies the elements a lane reaches after its first (i >= 64) by 0",
   "avgpool_fwd_kernel, the second lane turn (P > 64)",
   [RAG + "test_avgpool_second_lane_turn[f32]", RAG + "test_avgpool_second_lane_turn[bf16]"])
_m("softmax_max_of_first_64", "kernels_misc.hip",
   "for (int j = lane; j < L; j += 64) mx = fmaxf(mx, xr[j]);",
   "for (int j = lane; j < L; j += 64) mx = j >= 64 ? mx : fmaxf(mx, xr[j]);",
   "the row maximum of softmax_kernel ignores the columns from 64 on: the same function up to rounding unless a dominant logit sits there",
   "softmax_kernel, the maximum's second lane turn (L > 64)",
   [RAG + "test_softmax_dominant_logit_past_column_63[65]", RAG + "test_softmax_dominant_logit_past_column_63[1000]"])
_m("softmax_sum_second_turn_scaled", "kernels_misc.hip",
   "float s = 0.f;\n    for (int j = lane; j < L; j += 64) s += expf(xr[j] - mx);",
   "float s = 0.f;\n    for (int j = lane; j < L; j += 64) s += (j >= 64 ? 1.0009765625f : 1.f) * expf(xr[j] - mx);",
   "the sum of softmax_kernel scales the terms a lane adds after its first by 1 + 2^-10",
   "softmax_kernel, the sum's second lane turn (L > 64)",
   [RAG + "test_pools_softmax_fc_ragged[r50_N8-softmax_ce_deriv]"])
_m("adam_second_turn_v_corrected_with_beta1", "kernels_misc.hip",
   "const float ma = mi / (1.f - cur_b1), va = vi / (1.f - cur_b2);",
   "const float ma = mi / (1.f - cur_b1), va = vi / (1.f - (i >= (size_t)gridDim.x * blockDim.x ? cur_b1 : cur_b2));",
   "elements a thread of adam_kernel reaches after its first (i >= 16384 x 256) have the second moment corrected with beta1^t",
   "adam_kernel, the second grid-stride turn (n > 4 194 304)",
   [OPS + "test_adam_second_grid_stride_turn"])
_m("adam_no_decoupled_decay", "kernels_misc.hip",
   "float np = old - (lr * (ma / (sqrtf(va) + eps)) + wd * old);",
   "float np = old - (lr * (ma / (sqrtf(va) + eps)) + 0.f * wd * old);",
   "the parameter update of adam_kernel lacks the decoupled wd * old term",
   "adam_kernel, wd > 0",
   [OPS + "test_softmax_ce_adam"])

_m("relu_deriv_gate_ge", "kernels_misc.hip",
   "a.x > 0.f ? u.x : 0.f",
   "a.x >= 0.f ? u.x : 0.f",
   "relu_deriv_kernel passes the upstream gradient where the activation is exactly 0, in the first element of every float4",
   "relu_deriv_kernel (mi_op_relu_deriv), the float4 body",
   [OPS + "test_bn_add_relu_and_external_mask[256-8-4]"])

_m("add_relu_activation_without_addend", "kernels_misc.hip",
   "act_out[i] = fmaxf(0.f, s);",
   "act_out[i] = fmaxf(0.f, a[i]);",
   "add_relu_kernel's activation is max(a, 0): the shortcut is missing from the block output (the stored sum keeps it)",
   "add_relu_kernel (the expansion's add + ReLU as a pass of its own: the trainer's FULL store policy)",
   [OPS + "test_full_store_policy_tensors_per_element"])

# kernels_optim.hip, the optimizer half
_m("optim_norm_whole_chunk_last_quad_g_zero", "kernels_optim.hip",
   "q[k] = ((const float4 *)pg)[threadIdx.x + k * OPT_THREADS];",
   "q[k] = k == MID_OPT_CHUNK / 4 / OPT_THREADS - 1 ? make_float4(0.f, 0.f, 0.f, 0.f) : ((const float4 *)pg)[threadIdx.x + k * OPT_THREADS];",
   "the whole-chunk branch of optim_norm_kernel takes the gradients of its last load per thread (k == K - 1) as 0: an eighth of sum g^2",
   "optim_norm_kernel, whole chunks of 8192 floats",
   [OPT + "test_operator_scalar_tail[lars]"])
_m("optim_norm_partial_second_turn_zero", "kernels_optim.hip",
   "const float4 w = ((const float4 *)pw)[i], q = ((const float4 *)pg)[i];",
   "const float4 z_ = make_float4(0.f, 0.f, 0.f, 0.f), w = i >= OPT_THREADS ? z_ : ((const float4 *)pw)[i], q = i >= OPT_THREADS ? z_ : ((const float4 *)pg)[i];",
   "the float4 loop of a partial chunk of optim_norm_kernel takes the quads a thread reaches after its first (i >= 256) as 0",
   "optim_norm_kernel, partial chunks of more than 1024 floats",
   [OPT + "test_operator_scalar_tail[lars]"])
_m("optim_norm_interwave_wave3_dropped", "kernels_optim.hip",
   "for (int k = 0; k < OPT_THREADS / 64; k++) { a += red[0][k]; b += red[1][k]; }",
   "for (int k = 0; k < OPT_THREADS / 64; k++) { a += k == 3 ? 0.0 : red[0][k]; b += k == 3 ? 0.0 : red[1][k]; }",
   "the inter-wave sum of optim_norm_kernel leaves the fourth wave out",
   "optim_norm_kernel, the sum over the four waves",
   [OPT + "test_operator_scalar_tail[lars]"])
_m("optim_trust_second_lane_turn_zero", "kernels_optim.hip",
   "{ sw += part[c].x; sg += part[c].y; }",
   "{ sw += c - first_chunk[t] >= 64 ? 0.0 : part[c].x; sg += c - first_chunk[t] >= 64 ? 0.0 : part[c].y; }",
   "optim_trust_kernel takes the partials a lane reaches after its first (chunk 64 and up of a tensor) as 0",
   "optim_trust_kernel, the second lane turn (tensors of more than 64 chunks: more than 524 288 floats)",
   [OPT + "test_operator_per_element_at_resnet50_geometry[lars-5e-05]"])
_m("optim_trust_guard_gn_only", "kernels_optim.hip",
   "if (wn > 0.f && gn > 0.f) tr",
   "if (gn > 0.f) tr",
   "the trust-1 guard of optim_trust_kernel looks at the gradient norm alone: an all-zero weight tensor gets trust ratio 0 and never moves",
   "optim_trust_kernel, wn == 0 with gn > 0",
   [OPT + "test_lars_loop_turns_and_an_all_zero_weight_tensor"])
_m("optim_update_whole_chunk_last_w_no_decay", "kernels_optim.hip",
   "opt_elem<KIND>(w[k].w, q[k].w, b[k].w, s, wdt, lr, mu, skip, bad);",
   "opt_elem<KIND>(w[k].w, q[k].w, b[k].w, s, k == K - 1 ? 0.f : wdt, lr, mu, skip, bad);",
   "the whole-chunk path of optim_update_kernel runs the .w element of a thread's last quad without weight decay: one element in 32",
   "optim_update_kernel, whole chunks, wd > 0",
   [OPT + "test_operator_scalar_tail[sgd]", OPT + "test_operator_per_element_at_resnet50_geometry[sgd-5e-05]"])
_m("optim_update_partial_second_turn_no_momentum", "kernels_optim.hip",
   "float4 w = ((float4 *)pw)[i], q = ((float4 *)pg)[i], b = ((float4 *)pb)[i];",
   "float4 w = ((float4 *)pw)[i], q = ((float4 *)pg)[i], b = ((float4 *)pb)[i];\n            if (i >= OPT_THREADS) b = make_float4(0.f, 0.f, 0.f, 0.f);",
   "the partial-chunk path of optim_update_kernel reads the momentum of the quads a thread reaches after its first as 0 (mu b = 0)",
   "optim_update_kernel, partial chunks of more than 1024 floats",
   [OPT + "test_operator_scalar_tail[sgd]"])

# kernels_loss.hip
_m("loss_reg_max_of_first_slot", "kernels_loss.hip",
   "if (j < L) { v[k] = xr[j]; mx = fmaxf(mx, v[k]); }",
   "if (j < L) { v[k] = xr[j]; mx = k >= 1 ? mx : fmaxf(mx, v[k]); }",
   "the row maximum of loss_head_kernel<reg> ignores the register slots k >= 1 (columns from 64 on)",
   "loss_head_kernel<reg>, the maximum over the slots (64 < L <= 1024)",
   # pred must have the soft-max operator's bits: another maximum is another rounding
   [LOSS + "test_loss_head[shape4-0.1]"])
_m("loss_mem_max_of_first_64", "kernels_loss.hip",
   "for (int j = lane; j < L; j += 64) mx = fmaxf(mx, xr[j]);",
   "for (int j = lane; j < L; j += 64) mx = j >= 64 ? mx : fmaxf(mx, xr[j]);",
   "the row maximum of loss_head_kernel<mem> ignores the columns from 64 on",
   "loss_head_kernel<mem>, the maximum loop (L > 1024)",
   [LOSS + "test_loss_head[shape5-0.1]"])
_m("loss_reg_rank_last_slot_left_out", "kernels_loss.hip",
   "if (j < L) LOSS_COLUMN(j, v[k]);",
   "if (j < L) { const int keep_ = above; LOSS_COLUMN(j, v[k]); above = k == NV - 1 ? keep_ : above; }",
   "the rank of loss_head_kernel<reg> does not count the columns of the last register slot (960 .. 1023)",
   "loss_head_kernel<reg>, slot k == NV - 1 (L > 960)",
   [LOSS + "test_loss_head[shape4-0.0]"])

# kernels_input.hip: the decode and the plain resample (resample_aa_u8_kernel's turns have their entries above)
_m("decode_stage_second_turn_zero", "kernels_input.hip",
   "        if (a < g + span) *(uint4 *)(rows + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);\n    }\n    __syncthreads();",
   "        if (a < g + span) *(uint4 *)(rows + ((size_t)r * CH + c) * 16) = i >= DEC_THREADS ? make_uint4(0u, 0u, 0u, 0u) : load16_in_batch(src, a, total_bytes);\n    }\n    __syncthreads();",
   "the 16-byte pieces a thread of decode_u8_kernel stages after its first (i >= 256) are stored as zeros",
   "decode_u8_kernel, the second turn of the staging loop (16 CH > 256: dim_out >= 81)",
   [U8 + "test_decode_sweep[256-224-1]"])
_m("decode_second_quad_turn_plus_one", "kernels_input.hip",
   "for (int p = 0; p < 3; p++) v[p][j] = tab[p * 256 + L[px * 3 + p]];",
   "for (int p = 0; p < 3; p++) v[p][j] = tab[p * 256 + L[px * 3 + p]] + (i >= DEC_THREADS ? 1.f : 0.f);",
   "quads a thread of decode_u8_kernel reaches after its first (i >= 256) come out 1.0 high",
   "decode_u8_kernel, the second turn of the quad loop (16 (dim_out / 4) > 256: dim_out >= 68)",
   [U8 + "test_decode_sweep[256-224-1]"])
_m("decode_scalar_store_lane3", "kernels_input.hip",
   "                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j];\n            }\n        }\n    }\n    const int T = dim_out & 3;",
   "                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j] + (j == 3 ? 0.0625f : 0.f);\n            }\n        }\n    }\n    const int T = dim_out & 3;",
   "the element-wise store of a quad of decode_u8_kernel (vec == 0) adds 2^-4 to its fourth value",
   "decode_u8_kernel, the element-wise quad stores (dim_out % 4 != 0 or an unaligned out)",
   [U8 + "test_decode_sweep[40-33-1]"])
_m("resample_ctab_past_256_no_weight", "kernels_input.hip",
   "ctab[i] = (uint32_t)(fx >> 8) | (uint32_t)(fx & 255) << 16;",
   "ctab[i] = (uint32_t)(fx >> 8) | (uint32_t)(i >= RS_THREADS ? 0 : fx & 255) << 16;",
   "column-table entries a thread of resample_u8_kernel fills after its first (i >= 256) get horizontal weight 0",
   "resample_u8_kernel, the second turn of the column-table fill (dim_out > 256)",
   [RRC + "test_resample_wide_output_and_wide_box"])
_m("resample_stage_pieces_past_64_zero", "kernels_input.hip",
   "*(uint4 *)(rows + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);\n        }\n    }",
   "*(uint4 *)(rows + ((size_t)r * CH + c) * 16) = c >= 64 ? make_uint4(0u, 0u, 0u, 0u) : load16_in_batch(src, a, total_bytes);\n        }\n    }",
   "the 16-byte pieces of a source row that a lane of resample_u8_kernel stages after its first (c >= 64) are stored as zeros: source "
   "bytes from 1024 on, counted from the span's start rounded down to 16",
   "resample_u8_kernel, the second lane turn of the staging loop (boxes of 337 columns and more)",
   [RRC + "test_resample_wide_output_and_wide_box"])
_m("resample_scalar_store_lane3", "kernels_input.hip",
   "                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j];\n            }\n        }\n    }\n    const int T = D & 3;",
   "                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j] + (j == 3 ? 0.0625f : 0.f);\n            }\n        }\n    }\n    const int T = D & 3;",
   "the element-wise store of a quad of resample_u8_kernel (vec == 0) adds 2^-4 to its fourth value",
   "resample_u8_kernel, the element-wise quad stores",
   [RRC + "test_resample_sweep[40-33-1]", RRC + "test_resample_into_an_unaligned_output"])
_m("resample_second_quad_turn_plus_one", "kernels_input.hip",
   "for (int p = 0; p < 3; p++) v[p][j] = rs_value(L0, L1, x0, x1, wx, wy, p);",
   "for (int p = 0; p < 3; p++) v[p][j] = rs_value(L0, L1, x0, x1, wx, wy, p) + (i >= RS_THREADS ? 1.f : 0.f);",
   "quads a thread of resample_u8_kernel reaches after its first (i >= 256) come out 1.0 high",
   "resample_u8_kernel, the second turn of the quad loop (R (dim_out / 4) > 256)",
   [RRC + "test_resample_sweep[256-224-1]"])

# mi_common.hpp (one header mutant: it recompiles every .hip file)
_m("pack_bf2_truncates", "mi_common.hpp",
   "    bf2_ r = __builtin_convertvector(v, bf2_);\n    return *(uint32_t *)&r;",
   "    (void)v; (void)sizeof(bf2_);\n    return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);",
   "mi_pack_bf2 truncates: every bf16 store of the batch-norm, pooling and stem kernels",
   "bf16 storage",
   [RAG + "test_bn_fwd_ragged[c1s_N4-bf16_C64_H8]"])

KERNEL_FILES = ["kernels_bn.hip", "kernels_cl_bf16.hip", "kernels_conv.hip", "kernels_gemm.hip", "kernels_igemm.hip", "kernels_igemm_bf16.hip",
                "kernels_input.hip", "kernels_loss.hip", "kernels_misc.hip", "kernels_optim.hip", "kernels_stem_bf16.hip"]


def by_name(name):
    for m in MUTANTS:
        if m["name"] == name:
            return m
    raise KeyError(name)


def all_killers():
    seen = []
    for m in MUTANTS:
        for k in m["killers"]:
            if k not in seen:
                seen.append(k)
    return seen
