"""The CPU oracle's own self-noise on the second optic of the relay tests (tests/test_gpu_relay.py): no GPU involved.

    python scripts/relay_floors.py [--tilt TILT_X TILT_Y] [--offset OFF_X OFF_Y]

For each configuration of the tests: the oracle traces optic A (seed 20000, slots 0..19999, images kept), the exit records are flown
to B's entrance by the numpy restatement of the relay contract (gap 1 cm, aligned), and the oracle's launch_batch on B is compared
with itself after one start coordinate has been moved by 1 ulp -- x up, x down, y up, y down.  Printed per configuration: the share
of photons whose return code or reflection count flips, and |delta| / sum * sqrt(n) of the transmitted product weight (largest over
the energies), for each of the four and their maxima, which are the floors the tests use.  With --tilt (rad) and --offset (cm) B is
posed as a tilted relay poses it (tests/test_gpu_relay_pose.py): the numpy restatement of that contract flies the records, with the
basis the library computes on the host, and the photons that miss B's entrance plane are left out."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPE_B = (2, 9., 0.0585, 0.2065, 9.9153e-5, 0.00035, 0.5, 1000.)          # tests/common.py:TEST_SHAPE reversed
SRC = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)
CONFIGS = {"pinned": ((10.0,), 0.), "ne12": (tuple(np.linspace(5., 27., 12)), 0.), "rough": ((10.0,), 5.)}


def floors(oracle, name, seed=20000, n=20000, gap=1.0, tilt=(0., 0.), offset=(0., 0.)):
    """(flip shares [4], weight c [4], rc-1 count) of configuration `name`"""
    from tests.common import make_custom, make_pair
    from tests.test_relay_cpu import np_fly
    en, rough = CONFIGS[name]
    optic_a, src, _, (E, A, S) = make_pair(oracle, "ellip", energies=en)
    optic_b, _, _, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=en, sig_rough=rough)
    o = oracle.transmission(optic_a, src, E, A, S, seed, 0, n, images=True)
    im, wa = o["images"], o["exit_weights"]
    if tuple(tilt) == (0., 0.) and tuple(offset) == (0., 0.):
        f = np_fly(im[:, 8], im[:, 9], im[:, 11], im[:, 12], im[:, 13], im[:, 14], gap, 0., 0.)
    else:
        import polycap_amd
        from tests.test_relay_pose_cpu import np_fly_posed
        f, hit = np_fly_posed(im[:, 8], im[:, 9], im[:, 11], im[:, 12], im[:, 13], im[:, 14], gap, offset[0], offset[1],
                              polycap_amd.relay_basis(gap, offset, tilt))
        f, wa = f[hit], wa[hit]
    a = oracle.launch_batch(optic_b, E, A, S, f[:, 0:3], f[:, 3:6], f[:, 6:9])
    ent = np.isin(a["rc"], (2, -2))
    sa = (wa * a["weights"])[a["rc"] == 1].sum(axis=0)
    flips, cs = [], []
    for col in (0, 1):
        for to in (1.0, -1.0):
            st = f[:, 0:3].copy()
            st[:, col] = np.nextafter(st[:, col], to)
            b = oracle.launch_batch(optic_b, E, A, S, st, f[:, 3:6], f[:, 6:9])
            assert np.array_equal(ent, np.isin(b["rc"], (2, -2))) and np.array_equal(a["rc"][ent], b["rc"][ent])   # entrance decisions hold
            flips.append(float(((a["rc"] != b["rc"]) | (a["i_refl"] != b["i_refl"])).mean()))
            sb = (wa * b["weights"])[b["rc"] == 1].sum(axis=0)
            cs.append(float((np.abs(sa - sb) / sa * np.sqrt(n)).max()))
    return flips, cs, int((a["rc"] == 1).sum())


if __name__ == "__main__":
    import argparse
    from oracle import pyoracle
    ap = argparse.ArgumentParser()
    ap.add_argument("--tilt", type=float, nargs=2, default=(0., 0.), metavar=("TILT_X", "TILT_Y"))
    ap.add_argument("--offset", type=float, nargs=2, default=(0., 0.), metavar=("OFF_X", "OFF_Y"))
    args = ap.parse_args()
    pyoracle.build()
    for name in CONFIGS:
        fl, cs, n1 = floors(pyoracle, name, tilt=tuple(args.tilt), offset=tuple(args.offset))
        print("%-7s rc 1 %5d  flips %s  max %.5f   c %s  max %.4f" % (name, n1, ["%.5f" % v for v in fl], max(fl), ["%.4f" % v for v in cs], max(cs)))
