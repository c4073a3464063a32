"""Row strides of the D = 192 staged temporal-attention tiles (csrc/vda_attn.hip temporal_attn_lds192_kernel), by
brute force over the LDS bank rules of gfx950: the bank of byte address a is (a / 4) % 64 for ds_read_b128 and
ds_read_b64_tr_b16; a ds_read_b128 is served in four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32),
a ds_read_b64_tr_b16 in two 32-lane halves; distinct addresses on one bank within a group cost a cycle each.

A row is 24 16-byte chunks of data; the stride is CS chunks.  Prints, per CS, the worst number of distinct addresses on
one bank (1 = conflict-free) for the K / Q fragment reads and for the transposed V reads, and the LDS of a tile.

    python tools/ta192_stride.py
"""
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]
TR_GROUPS = [list(range(32)), list(range(32, 64))]


def worst(groups, addr, nbytes):
    """Max over groups and banks of the number of distinct dword addresses on a bank."""
    w = 0
    for g in groups:
        banks = {}
        for lane in g:
            a = addr(lane)
            for dw in range(a // 4, (a + nbytes) // 4):
                banks.setdefault(dw % 64, set()).add(dw)
        w = max(w, max(len(v) for v in banks.values()))
    return w


def kq_reads(cs):  # lane (r32, hf) reads row r32, chunk 2 st + hf
    return max(worst(B128_GROUPS, lambda l: ((l & 31) * cs + 2 * st + (l >> 5)) * 16, 16) for st in range(12))


def v_reads(cs):  # ta_vpos: rows 16 st + 4 (grp >> 1) + q4 (and + 8), columns 32 dt + 16 (grp & 1) + 4 p4
    w = 0
    for dt in range(6):
        for st in range(2):
            for up in (0, 8):
                def addr(l):
                    grp, q4, p4 = l >> 4, (l & 15) >> 2, l & 3
                    return ((16 * st + 4 * (grp >> 1) + q4 + up) * cs * 8 + dt * 32 + (grp & 1) * 16 + 4 * p4) * 2
                w = max(w, worst(TR_GROUPS, addr, 8))
    return w


if __name__ == "__main__":
    print("chunks/row  stride B  K/Q b128 reads  V tr16 reads  tile KiB (whole 1-KiB DMA instructions)")
    for cs in range(24, 33):
        print(f"{cs:10d}  {cs * 16:8d}  {kq_reads(cs):14d}  {v_reads(cs):12d}  {-(-32 * cs // 64):8d}")
