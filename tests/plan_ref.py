"""Python restatement of the split-K plans of the weight-gradient products (csrc/splitk.h splitk_plan over common.h
pe_pick_splits, with each entry point's tile choice), for tests that must know which tile and how many k-splits a
shape takes.  tests/test_splitk_plan_cpu.py holds the library to the same numbers through its workspace queries."""

K_TILE = 32                                            # gemm_engine.h kBK


def cdiv(a, b):
    return -(-a // b)


def pick_splits(tiles, K, min_k, resident):            # common.h pe_pick_splits
    max_s = min(max(K // min_k, 1), 1024)
    best, best_score = 1, -1.0
    for sp in range(1, max_s + 1):
        wgs = tiles * sp
        waves = (wgs + resident - 1) // resident
        score = wgs / (waves * resident) - 0.0001 * sp + (0.05 if wgs >= 2 * resident else 0.0)
        if score > best_score:
            best, best_score = sp, score
    return best


def splitk_plan(tiles, K, min_k, resident):
    """(splits, k per split) of splitk.h splitk_plan"""
    kps = cdiv(cdiv(K, pick_splits(tiles, K, min_k, resident)), K_TILE) * K_TILE
    return cdiv(K, kps), kps


def tn_resident(multi_term):
    """workgroups the TN engine keeps resident: x3 / h2 (multi-term LDS images) 512, native / bf16 / f16 768"""
    return 512 if multi_term else 768


def tn_tile_and_splits(M, N, K, multi_term=False):
    """(BM, BN) and k-splits gemm_tn_impl chooses (default: for a 16-bit operand product)"""
    bm, bn = (64, 64) if M <= 64 and N <= 64 else (64, 128) if M <= 64 else (128, 64) if N <= 64 else (128, 128)
    return (bm, bn), splitk_plan(cdiv(M, bm) * cdiv(N, bn), K, 512, tn_resident(multi_term))[0]


def whh_splits(B, T, H, multi_term=False):
    """k-splits of pe_lstm_whh_grad: the 128 x 128 tile at every H"""
    return splitk_plan(cdiv(4 * H, 128) * cdiv(H, 128), B * T, 512, tn_resident(multi_term))[0]


def wgrad_tile_and_splits(P, Cout, Cin):
    """(BM, BN) and k-splits of csrc/conv.hip wgrad_plan over P = B T F pixels"""
    nine = Cout % 64 == 0 and Cin % 64 == 0
    bm, bn = (64 if nine or Cout <= 64 else 128), (64 if nine or Cin <= 64 else 128)
    tiles = cdiv(Cout, bm) * cdiv(Cin, bn) * (1 if nine else 9)
    return (bm, bn), splitk_plan(tiles, P, 1024, 512 if nine else 768)[0]
