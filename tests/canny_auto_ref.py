"""CPU oracle of the automatic Canny thresholds (the contract: the comment of i2i_canny_auto_thr_params in include/i2i_turbo.h): the median
rule low = (1 - sigma) * median, high = (1 + sigma) * median in integers, with numpy's sort as the order statistics.  The rule is not part
of the reference; the integer form below IS the contract, and float_rule() is the widely used float form it restates (the two differ by at
most 1: tests/test_canny_auto_emu.py::test_integer_rule_matches_float_rule)."""
import numpy as np


def median2(img):
    """a + b over ALL bytes of the image (every channel): a = the order statistic of 0-based rank (N - 1) // 2, b = the one of rank N // 2.
    Exactly 2 * np.median(img)."""
    flat = np.sort(np.asarray(img, dtype=np.uint8).reshape(-1))
    n = flat.size
    return int(flat[(n - 1) // 2]) + int(flat[n // 2])


def thresholds(m2, sigma_q16):
    """(low, high) of a doubled median under sigma * 65536 (clamped to 65536 from above)."""
    s = min(int(sigma_q16), 65536)
    return max(0, (m2 * (65536 - s)) >> 17), min(255, (m2 * (65536 + s)) >> 17)


def auto_thresholds(images, sigma_q16, thr=None, med=None):
    """The op on a batch [n, h, w, c]: returns (thr int32 [n, 2], median2 uint32 [n]); rows with a negative sigma keep what ``thr`` /
    ``med`` hold (zeros if not given)."""
    n = len(images)
    thr = np.zeros((n, 2), dtype=np.int32) if thr is None else np.array(thr, dtype=np.int32).reshape(n, 2)
    med = np.zeros(n, dtype=np.uint32) if med is None else np.array(med, dtype=np.uint32).reshape(n)
    for b in range(n):
        if sigma_q16[b] < 0:
            continue
        m2 = median2(images[b])
        thr[b] = thresholds(m2, sigma_q16[b])
        med[b] = m2
    return thr, med


def float_rule(m2, sigma):
    """The float form of the rule on the same doubled median."""
    median = m2 / 2.0
    return int(max(0, (1.0 - sigma) * median)), int(min(255, (1.0 + sigma) * median))
