# CPU model of hist_lean.hip's predict_hybrid: sample positions, generator (kernels.hip k_fill), rule
import numpy as np
M=np.uint64
def mix64(z):
    z = z + M(0x9E3779B97F4A7C15)
    z = (z ^ (z >> M(30))) * M(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> M(27))) * M(0x94D049BB133111EB)
    return z ^ (z >> M(31))
def gen(pos, seed, dist, n):
    gi = pos.astype(np.uint64)
    z = mix64(M(seed) ^ (gi * M(0x9E3779B97F4A7C15)))
    hi = (z >> M(32)).astype(np.uint32)
    if dist=="u32": return hi
    if dist=="u31": return (z >> M(33)).astype(np.uint32)
    if dist=="mod1000": return hi % np.uint32(1000)
    if dist=="sorted": return gi.astype(np.uint32)
def positions(n):
    r = np.arange(256, dtype=np.uint64)
    span = n // 256
    room = span - 63
    off = ((r * M(2654435761)) & M(0xFFFFFFFF)) >> M(8)
    start = r * M(span) + off % M(room)
    return (start[:,None] + np.arange(64,dtype=np.uint64)[None,:]).ravel()
def predict(keys, n, limit):
    a = np.bitwise_and.reduce(keys); o = np.bitwise_or.reduce(keys); d = int(a ^ o)
    bins = np.bincount(keys >> np.uint32(28), minlength=16)
    maxc = int(bins.max())
    thr = 5*limit*16384*1024/(4*n)
    likely = (d & 255)!=0 and ((d>>8)&255)!=0 and maxc*n*4 <= 5*limit*16384*1024
    return likely, maxc, thr
LIM=20480
with np.errstate(over='ignore'):
    for n,dist in [(15<<24,"u32"),(1<<28,"u32"),(19<<24,"u32"),(1<<28,"u31"),(1<<28,"sorted"),(1<<28,"mod1000")]:
        for seed in (0x5EED0003, 1, 2, 3):
            k = gen(positions(n), seed, dist, n)
            l, maxc, thr = predict(k, n, LIM)
            print(f"n={n/(1<<24):5.1f}x2^24 {dist:8s} seed={seed:#x} likely={l} max bin {maxc} threshold {thr:.1f}")
    # margin at 19 x 2^24: distribution of the largest of 16 bins over many uniform samples
    rng = np.random.default_rng(1)
    mx = np.array([np.bincount(rng.integers(0,16,16384),minlength=16).max() for _ in range(20000)])
    thr = 5*LIM*16384*1024/(4*(19<<24))
    print("u32, 20000 samples: largest bin mean %.1f max %d; threshold at 19x2^24 %.1f (bin sd %.1f -> %.1f sd above the mean bin 1024)" % (mx.mean(), mx.max(), thr, (16384*15/256)**.5, (thr-1024)/(16384*15/256)**.5))
    mn = np.array([np.bincount(rng.integers(0,8,16384),minlength=8).max() for _ in range(20000)])
    print("u31 at 2^28: largest bin min %d, threshold %.1f" % (mn.min(), 5*LIM*16384*1024/(4*(1<<28))))
