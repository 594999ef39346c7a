"""The launch policy of the contraction kernel (renormalizer_amd/csrc/mpse_plans.h: launch_plan, grouped_plan) restated in
Python, and the table of launch paths built on it.  tests/test_gemm_gpu.py asserts the path counters of real launches
against it; tests/test_gemm_plan_host.py asserts the C plans against it without a GPU.
"""
import math


def _ksplit(base, nkt, n_cu):
    """K slices of a product with `base` output tiles (the split rule of gemm_impl), 1 = unsplit"""
    if base >= n_cu or nkt < 4:
        return 1
    s = min(-(-n_cu // base), nkt // 2)
    if s <= 1:
        return 1
    per = -(-nkt // s)
    return -(-nkt // per)


# ------------------------------------------------------------------------------------------------ the table of tests/test_gemm_gpu.py
def _four_wave_dims(n_cu):
    tn = max(n_cu // 18 + 1, 4)                       # (at least 64 tiles: past the threshold of the die grouping)
    tn += tn % 8 == 0
    return 64 * 18 - 52, 64 * tn - 60, 24, 1          # 18 x tn tiles > n_cu, neither side a multiple of 8


def _tile_order_dims(n_cu):
    t = max(25, math.isqrt(2 * n_cu) + 1)
    t += t % 8 == 0
    assert t * t <= 2048
    return 64 * t, 64 * t, 64, 1                      # t * t tiles: above 2 n_cu, at most 2048


def _first_below(n_cu, *shapes):
    """the first (M, N, K, batch) with fewer output tiles, times batch, than compute units: few enough for its row"""
    for M, N, K, batch in shapes:
        if -(-M // 64) * -(-N // 64) * batch < n_cu:
            return M, N, K, batch
    raise AssertionError(f"no shape of the row fits {n_cu} compute units")


def _die_tiles(n_cu):
    """tiles (a multiple of 8) along the grouped side of the die-group rows, 5 along the other: at least 64 tiles, and
    at most 2 n_cu, from where a launch with masks is sorted instead - or, where both cannot hold, more than the 2048
    tiles a sort takes"""
    return 32 if 160 <= 2 * n_cu else 16 if 80 <= 2 * n_cu else 416


# name: (dims(n_cu) -> (M, N, K, batch), layout, block sparse, skip hints, alpha, beta)
CASES = {
    "eight_wave": (lambda n: _first_below(n, (300, 200, 40, 1), (300, 64, 40, 1)), "rowmajor", False, (0,), 1, 0),
    "four_wave": (_four_wave_dims, "rowmajor", False, (0,), 2, -1),
    "split_b1": (lambda n: (100, 90, 3000, 1), "rowmajor", False, (0,), 2 - 1j, 3 + 2j),
    "split_batched": (lambda n: _first_below(n, (70, 130, 2000, 3), (60, 100, 2000, 3)), "gaps", False, (0,), -1 + 1j, 0.5),
    "die_group1": (lambda n: (64 * _die_tiles(n), 300, 32, 1), "rowmajor", True, (0, 1, 2, 3), 1, 1),
    "die_group1_ragged": (lambda n: (64 * _die_tiles(n) - 48, 300, 32, 1), "rowmajor", True, (0, 1, 2, 3), 0.25, -2),
    "die_group2": (lambda n: (300, 64 * _die_tiles(n) - 48, 32, 1), "rowmajor", True, (0, 1, 2, 3), 1j, 1),
    "die_group1_fallback": (lambda n: (512, 1100, 8, 1), "rowmajor", False, (0,), 1, 2),
    "tile_order": (_tile_order_dims, "rowmajor", True, (0, 1, 2, 3), 2 + 1j, -1j),
    "masks_global": (lambda n: (100, 90, 9000, 1), "rowmajor", True, (0, 3), 1, -1),
    "masks_transposed": (lambda n: _first_below(n, (300, 200, 520, 1), (100, 90, 520, 1)), "trans", True, (0, 1, 2, 3), -2, 1 + 1j),
    "general_twolevel": (lambda n: _first_below(n, (300, 301, 299, 1), (100, 133, 299, 1)), "twolevel", False, (0,), 1 - 1j, 2),
    "general_reversed": (lambda n: _first_below(n, (200, 150, 100, 1), (100, 150, 100, 1)), "reversed", False, (0,), 3, 0.5j),
    "general_reversed_unsplit": (_four_wave_dims, "reversed", False, (0,), 1, 1),
    "general_span": (lambda n: (70, 50, 3, 1), "span", False, (0,), 1 + 2j, -1),
}


def expected_paths(name, n_cu, M, N, K, batch, hint):
    """the counter deltas of one launch of case `name`"""
    tiles = -(-M // 64) * -(-N // 64)
    nkt = -(-K // 16)
    ks = _ksplit(tiles * batch, nkt, n_cu)
    wide = tiles * batch * ks <= n_cu and nkt >= 2
    masks = hint != 0
    e = {"launches": 1}
    if name == "eight_wave":
        e.update(eight_wave=1, skew=1)
    elif name == "four_wave":
        e.update(skew=1)
    elif name == "split_b1":
        e.update(split_b1=1, skew=1, eight_wave=int(wide))
    elif name == "split_batched":
        e.update(split_batched=1, skew=1, eight_wave=int(wide))
    elif name in ("die_group1", "die_group1_ragged", "die_group2"):
        e.update({"die_group2" if name == "die_group2" else "die_group1": 1, "eight_wave": int(wide),
                  "masks": int(masks)})
    elif name == "die_group1_fallback":
        e.update(die_group1=1)
    elif name == "tile_order":
        e.update(tile_order=1, masks=1) if masks else e.update(skew=1)
    elif name in ("masks_global", "masks_transposed"):
        e.update(split_b1=1, skew=1, eight_wave=int(wide), masks=int(masks))
        if name == "masks_global":
            e.update(masks_global=int(masks))
    elif name in ("general_twolevel", "general_reversed"):
        e.update(general=1, split_b1=1, skew=1)
    elif name in ("general_reversed_unsplit", "general_span"):
        e.update(general=1, skew=1)
    return {k: v for k, v in e.items() if v}


def _shape_preconditions(name, n_cu, M, N, K, batch):
    """the shape reaches its row of the table for this n_cu (a failure here means the table needs new sizes)"""
    tm, tn, nkt = -(-M // 64), -(-N // 64), -(-K // 16)
    ks = _ksplit(tm * tn * batch, nkt, n_cu)
    if name.startswith("split") or name.startswith("masks") or name in ("general_twolevel", "general_reversed"):
        assert ks > 1
    if name == "split_batched":
        assert batch > 1
    if name == "eight_wave":
        assert ks == 1 and tm * tn <= n_cu and nkt >= 2
    if name.startswith("die_group") or name in ("four_wave", "tile_order", "general_reversed_unsplit"):
        assert ks == 1 and tm * tn >= 64
    if name == "four_wave":
        assert tm * tn > n_cu and tm % 8 and tn % 8
    if name == "masks_global":
        assert -(-nkt // 8) > 64


# ------------------------------------------------------------------------------------------------ the whole plan
# Every field of launch_plan / grouped_plan, written out on its own: not derived from mpse_plans.h, so that
# tests/test_gemm_plan_host.py holds two statements of the policy against each other.
def _die_group(tiles_m, tiles_n, size_a, size_b):
    """a die owns whole tile rows (1) or tile columns (2) of the larger operand, where they divide among 8 dies"""
    if tiles_m * tiles_n < 64:
        return 0
    if size_a >= size_b and tiles_m % 8 == 0:
        return 1
    if tiles_n % 8 == 0:
        return 2
    return 1 if tiles_m % 8 == 0 else 0


def plain_plan(n_cu, M, N, K, batch, ca=False, cb=False, hint=0, k_single=True, fast_ok=True, dot_cap=None,
               slices_cap=None, beta=False):
    """every decision of one plain product.  dot_cap / slices_cap: None = no dot request / no eligible slice offer"""
    tm, tn, nkt = -(-M // 64), -(-N // 64), -(-K // 16)
    tiles = tm * tn
    base = tiles * batch
    ks = _ksplit(base, nkt, n_cu)
    per = -(-nkt // min(-(-n_cu // base), nkt // 2)) if ks > 1 else max(nkt, 1)
    ws_bytes = batch * ks * M * N * (16 if ca or cb else 8) if ks > 1 else 0
    leave = (ks > 1 and slices_cap is not None and dot_cap is None and batch == 1 and not beta
             and ws_bytes <= slices_cap)
    rgx, rgy = min(64, -(-N // 256)), min(32768, M * batch)
    producers = 0
    if dot_cap is not None and batch == 1:
        producers = base
        if ks > 1:                    # the reduction kernel forms the partials: its grid shrinks to the room there is
            cap_y = dot_cap // rgx
            if cap_y >= 1 and rgy > cap_y:
                rgy = cap_y
            producers = rgx * rgy
        if not 1 <= producers <= dot_cap:
            producers = 0
    masks = bool(hint) and k_single and nkt >= 2 and batch <= 16384
    order = batch == 1 and masks and tiles * ks > 2 * n_cu and tiles <= 2048
    die = _die_group(tm, tn, M * (2 if ca else 1), N * (2 if cb else 1)) if not order and ks == 1 and batch == 1 else 0
    fast = k_single and fast_ok
    return dict(tiles_m=tm, tiles_n=tn, nkt=nkt, ksplit=ks, kt_per_split=per, ws_bytes=ws_bytes, leave_slices=int(leave),
                nwg=base * ks, fast=int(fast), wide=int(fast and base * ks <= n_cu and nkt >= 2), masks=int(masks),
                nkw=-(-nkt // 8) if masks else 0, order=int(order), die_group=die, rgx=rgx, rgy=rgy,
                dot_producers=producers)


def paths_of_plan(p, batch):
    """the counters of mpse_gemm_path_stats one launch with plan `p` raises (zeros left out)"""
    masked = p["fast"] and p["masks"]
    e = dict(launches=1, general=1 - p["fast"], eight_wave=p["wide"], split_b1=int(p["ksplit"] > 1 and batch == 1),
             split_batched=int(p["ksplit"] > 1 and batch > 1), die_group1=int(p["die_group"] == 1),
             die_group2=int(p["die_group"] == 2), skew=int(not p["order"] and not p["die_group"]), tile_order=p["order"],
             masks=int(masked), masks_global=int(masked and p["nkw"] > 64))
    return {k: v for k, v in e.items() if v}


def grouped_plan(n_cu, M, N, ngrp, nkt_max, any_mask, split2, ca):
    """every decision of one grouped launch: ngrp groups of M rows, nkt_max K tiles in the longest group"""
    tm, tn = -(-M // 64) * ngrp, -(-N // 64)
    tiles = tm * tn
    nkw = -(-nkt_max // 8) if any_mask and -(-nkt_max // 8) <= 64 else 0
    order = nkw > 0 and (tiles > 2 * n_cu or split2) and tiles <= 2048
    die = _die_group(tm, tn, M * ngrp * (2 if ca else 1), N * 2) if not order else 0
    nwg = tiles * (2 if split2 else 1)
    return dict(tiles_m=tm, tiles_n=tn, nkw=nkw, die_group=die, order=int(order), wide=int(nwg <= n_cu), nwg=nwg)
