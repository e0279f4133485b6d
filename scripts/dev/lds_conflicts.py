"""LDS bank-conflict arithmetic for the blend backward kernels' matrix layouts (no GPU).

Rules: MI355X_MICROARCH.md, section LDS - ds_read_b128 is served in four 16-lane groups with banks (a/4) mod 64,
ds_read_b32 / ds_write_b32 in two 32-lane groups with banks (a/4) mod 32; identical addresses broadcast; each extra
distinct address on a busy bank adds one cycle.  Prints cycles per wave-instruction (ideal 4 resp. 2) for the A-operand
reads, the result-tile writes and the read-out of gs2d_backward.hip / gs3d_backward.hip under candidate strides.
"""
import itertools

G128 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
        list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
        list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
        list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
G32 = [list(range(0, 32)), list(range(32, 64))]


def cycles(addr_dwords, groups, width, mod, active=None):
    """addr_dwords[lane] -> first dword; width dwords per lane"""
    total = 0
    for g in groups:
        banks = {}
        for l in g:
            if active is not None and not active(l):
                continue
            a = addr_dwords(l)
            for k in range(width):
                banks.setdefault((a + k) % mod, set()).add(a + k)
        total += max([len(v) for v in banks.values()], default=1)
    return total


def report(name, xs, ds, koff):
    a_read = lambda m: (lambda l: (l & 15) * xs + koff * (l >> 4) + (16 if koff == 4 else 4) * m)
    r = [cycles(a_read(m), G128, 4, 64) for m in range(4)]
    w = [cycles(lambda l, i=i: (4 * (l >> 4) + i) * ds + (l & 15), G32, 1, 32) for i in range(4)]
    print(f"{name}: xstride {xs} dstride {ds} k-offset {koff}: A reads {r} (ideal 4), result writes {w} (ideal 2)")


def main():
    for xs, ds in itertools.product((68, 72), (17, 20)):
        report("2-D (kg offset 4 dwords)", xs, ds, 4)
    for xs in (68, 72):
        report("3-D (kg offset 16 dwords)", xs, 20, 16)
        report("3-D remapped (kg offset 4 dwords)", xs, 20, 4)


if __name__ == "__main__":
    main()
