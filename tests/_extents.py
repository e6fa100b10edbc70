"""The conv kernels' index arithmetic as a table of limits (helper, not a test): DESIGN.md, "Conv extents", restated independently.

operands(info) takes ONE conv step's stabnet_net_step_info() row (a dict, _route_census.Plan.info) and returns [(operand, extent
reached, limit)], all in floats and in Python integers: `extent reached` is the distance from the pointer the launch is bound with to
the end of everything its index arithmetic can form; `limit` is the largest extent for which that arithmetic is exact.  Nothing here
asks the library for a limit: the numbers below were read from the kernels (file:line beside each) and must be changed by hand, with
DESIGN.md, when a kernel's arithmetic changes.

    family (stabnet_net_step_info FAMILY)  kernel
    0       register-staged   conv_igemm_body.h       element offsets, `unsigned` from an `int` product
    1 2 3   ring              conv_ring_kernel.h      BYTE offsets, 4u * (unsigned)(int product)
    4 5     packed            conv_ring_kernel.h      the same A operand; weights from the image, 64-bit
    6       A-stationary      conv_astat_kernel.h     (size_t)row * x_ld; image 64-bit
    7       patch-stationary  conv_patch_kernel.h     (size_t)(int pixel) * x_ld; image 64-bit; own epilogue
    pair    (step kind 6)     conv_pair_kernel.h      (size_t)row * x_ld; residual `unsigned` from an `int` product
    b2b     (step kind 5)     conv_b2b_kernel.h       BYTE offsets for the input, the conv2 weights AND the residual
"""
INT = 1 << 31            # an `int` product is exact below 2^31; cast to `unsigned` it is then an exact element offset
BYTES32 = 1 << 30        # a 32-bit BYTE offset reaches 2^32 bytes = 2^30 floats
WIDE = 1 << 62           # size_t / long arithmetic: no limit of its own below the address space

FAMILY_IGEMM, FAMILY_RING, FAMILY_RING_KG, FAMILY_RING_PRO, FAMILY_PACKED, FAMILY_PACKED_KG2, FAMILY_ASTAT, FAMILY_PATCH = range(8)
RING_LIKE = (FAMILY_RING, FAMILY_RING_KG, FAMILY_RING_PRO, FAMILY_PACKED, FAMILY_PACKED_KG2)

S_CONV, S_CONV_B2B, S_CONV_PAIR = 1, 5, 6


def image_floats(cout, k):
    """conv_weight_image_floats (conv.hip): 3072 floats per (64-channel N tile, 32-deep K step)"""
    return -(-cout // 64) * (k // 32) * 3072


def input_limit(info, fused=None):
    fam, pixels = info["family"], (1 << 31) - 1
    if fused == "b2b":
        return BYTES32                                     # conv_b2b_kernel.h:201  a_voff = 4u * (unsigned)((..pixel..) * ld + cl * 4)
    if fused == "pair" or fam == FAMILY_ASTAT:
        return pixels * info["x_ld"]                       # conv_pair_kernel.h:126,135 / conv_astat_kernel.h:49  (size_t)row * x_ld, row an int
    if fam == FAMILY_PATCH:
        return pixels * info["x_ld"]                       # conv_patch_kernel.h:157  (size_t)(int pixel index) * x_ld
    if fam == FAMILY_IGEMM:
        return INT                                         # conv_igemm_body.h:72,75,130  (unsigned)(int product), elements
    assert fam in RING_LIKE, fam
    return BYTES32                                         # conv_ring_kernel.h:157 (row-run), 173  4u * (unsigned)(int product)


def weight_limit(info, fused=None):
    fam = info["family"]
    if fused == "b2b":
        return BYTES32                                     # conv_b2b_kernel.h:186  w2_voff = 4u * (unsigned)(row * K + cl * 4); conv3's rows: size_t (:247)
    if fam == FAMILY_IGEMM:
        return INT                                         # conv_igemm_body.h:90  (unsigned)(n * K + lc4 * 4)
    if fam in (FAMILY_RING, FAMILY_RING_KG, FAMILY_RING_PRO):
        return BYTES32                                     # conv_ring_kernel.h:160,186  4u * (unsigned)(n * K + cl * 4)
    return WIDE                                            # packed / A-stationary / patch read the image only (size_t: conv_ring_kernel.h:193,200,
                                                           # conv_astat_kernel.h, conv_patch_kernel.h:201); the OHWI rows are not touched


def residual_limit(info, fused=None):
    if fused == "b2b":
        return BYTES32                                     # conv_b2b_kernel.h:337,342,344  res_voff = roff * 4u + vec_voff: BYTES
    if info["reduce"]:
        return WIDE                                        # conv.hip:55,60  the reduce launch reads it, in size_t
    return INT                                             # conv_kernel.h:91,96 / conv_patch_kernel.h:71,76 / conv_pair_kernel.h:62  (unsigned)(m * res_ld)


def operands(info, fused=None):
    """[(operand, extent reached, limit)] of one conv step.  fused: None (the step as its own launch), "pair" (the conv3 half of a kind-6
    step: the row stabnet_net_step_info gives for it) or "b2b" (either half of a kind-5 step, from the rows of the plan without it)."""
    i = info
    assert i["kind"] in (S_CONV, S_CONV_PAIR), i["kind"]
    out = []
    in_reached = i["in_base"] + i["in_floats"] - i["in_off"]          # from the bound pointer to the end of the buffer: all X_LD columns
    assert in_reached >= (i["n"] * i["h"] * i["w"] - 1) * i["x_ld"] + i["cin"]
    out.append(("input", in_reached, input_limit(i, fused)))
    out.append(("weights", i["cout"] * i["k"], weight_limit(i, fused)))
    if i["w_image_off"] >= 0:
        out.append(("weight image", image_floats(i["cout"], i["k"]), WIDE))
    if i["res_off"] >= 0:
        assert i["res_floats"] >= i["n"] * i["res_h"] * i["res_w"] * i["res_ld"] - (i["res_ld"] - i["cout"])
        out.append(("residual", i["res_floats"], residual_limit(i, fused)))
    # every epilogue and the reduce launch store through (size_t)m * Cout + n (conv_kernel.h:135, conv_patch_kernel.h:110,
    # conv_pair_kernel.h:80, conv_b2b_kernel.h:105, conv.hip:76): the row index m is an int
    out.append(("output", i["out_floats"], ((1 << 31) - 1) * i["cout"]))
    out.append(("rows M", i["m"], (1 << 31) - 1))                     # conv_plan: a.M = a.N * a.Ho * a.Wo, an int
    out.append(("pixels N*H*W", i["n"] * i["h"] * i["w"], (1 << 31) - 1))
    if i["scratch_floats"]:
        out.append(("split-K slabs", i["scratch_floats"], WIDE))     # conv_kernel.h:73, conv.hip:41-45  (size_t)z * M * Cout
    return out


def violations(info, fused=None):
    """The operands of the step that are NOT inside their limit (extent reached <= limit)."""
    return [(op, n, lim) for op, n, lim in operands(info, fused) if n > lim]


# ---- the launch-time requirement of the training step's weight gradient (conv_bwd.hip:506), restated ------------------------------------
def wgrad_requirement_holds(N, H, W, Cin, Cout, KH, stride, pad):
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
    return N * Ho * Wo * Cout < (1 << 31) and (N * (H + 2 * pad) + 1) * (W + 2 * pad) * Cin < (1 << 31)

