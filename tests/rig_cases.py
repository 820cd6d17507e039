"""Shared by the rig-plan tests: the numpy restatement of k_rig_maps' region codes, the stand-in R of a chained step (an image whose
alpha is the union of the masks before it) and seeded mask sets for chains of any length."""
import numpy as np

PCT = 20   # pixflow_search_20
COLS, ROWS = 523, 261   # 136,503 pixels: no multiple of 4, so k_rig_maps' scalar tail runs
SEED_A, SEEDS = 1234, (1235, 1236, 1237, 1238)


def rig(synth, cols, rows, seed, n=5):
    top, imgs = synth.make_stitch_set(cols, rows, seed, n)
    return top.numpy(), [im.numpy() for im in imgs]


def rig_codes(top, Ls):
    """code_i = (L_i.a > 0 ? 100 : 0) + (u ? 50 : 0) with u the running union of top's and L_1 .. L_{i-1}'s alpha > 0"""
    u = top[..., 3] > 0
    maps = []
    for L in Ls:
        a = L[..., 3] > 0
        maps.append((a * np.uint8(100) + u * np.uint8(50)).astype(np.uint8))
        u = u | a
    return maps


def stand_ins(top, Ls):
    """R of every step as far as a plan can tell: step 1's is top, step i's an image with alpha 255 on top | L_1 | .. | L_{i-1}"""
    u = top[..., 3] > 0
    rs = [top]
    for L in Ls[:-1]:
        u = u | (L[..., 3] > 0)
        r = np.zeros_like(top)
        r[..., :3] = 90
        r[..., 3] = np.where(u, 255, 0)
        rs.append(r)
    return rs


def window_set(cols, rows, n, seed, gap_step=None):
    """top covers rows [0, 0.4 rows), L_i a random column window (with wrap) of rows [0.3 rows, rows): every step overlaps the running union
    in rows [0.3, 0.4).  gap_step = i makes L_i a window of the bottom rows that misses a union made to stay clear of it."""
    rs = np.random.RandomState(seed)
    x = np.arange(cols)[None, :]
    y = np.arange(rows)[:, None]

    def img(mask):
        im = rs.randint(16, 240, (rows, cols, 4)).astype(np.uint8)
        im[..., 3] = rs.choice(np.array([1, 128, 255], np.uint8), (rows, cols))
        im[~mask] = 0
        return im

    top = img((y < int(0.4 * rows)) & (x >= 0))
    Ls = []
    for i in range(n):
        x0, w = rs.randint(0, cols), rs.randint(cols // 8, cols // 3)
        inside = ((x - x0) % cols < w) & (y >= int(0.3 * rows))
        if gap_step is not None:
            if i < gap_step:
                inside = inside & (y < int(0.6 * rows))
            elif i == gap_step:
                inside = ((x - x0) % cols < w) & (y >= int(0.7 * rows))
        Ls.append(img(inside))
    return top, Ls
