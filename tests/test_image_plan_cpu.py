"""The image store's decisions without a GPU: the pure half of polycap_amd/csrc/hip/pc_images.h, compiled for the host
(tests/plan/images_host.cpp), against the rules restated here -- what a run stores and in how many launches, where an element of
each layout lies, which positions a group of compact blocks adds to a fetch, and the order of the caller's planes."""
import itertools

import pytest

from tests.plan.pyimages import COMPACT, NONE, PLANES, RECORDS, HipImages, Images

N_FIELDS = 17
MAX_PARTS = 16


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    im = Images(tmp_path_factory.mktemp("images_host"))
    assert (im.n_fields, im.max_parts) == (N_FIELDS, MAX_PARTS)
    return im


def _part_begin(n_slots, parts, k):
    """first slot of part k: with three or more parts the first and the last are half the size of the others"""
    if k <= 0:
        return 0
    if k >= parts:
        return n_slots
    if parts < 3:
        return n_slots * k // parts
    unit = 1.0 / float(parts - 1)
    return int(float(n_slots) * unit * (float(k) - 0.5))


def _parts(n_slots, keep, compact, run_parts, compact_parts):
    parts = run_parts if (keep and run_parts > 1 and not compact) else 1
    if compact and compact_parts > 1 and n_slots >= 4000000:
        parts = compact_parts
    if parts > MAX_PARTS:
        parts = MAX_PARTS
    if parts > n_slots // 65536:
        parts = n_slots // 65536
    if parts < 1:
        parts = 1
    return parts


GRID = list(itertools.product((1, 65535, 65536, 131071, 196608, 4 * 65536 + 17, 3999999, 4000000, 10000000), (0, 1),
                              ((0, 0), (1, 0), (1, 1), (0, 1)), (1, 2, 3, 4, 5, 16), (1, 2, 3)))


def test_plan_images_equals_the_rule(images):
    ne = 3
    seen = set()
    for n_slots, keep, (plane_images, compact_images), run_parts, compact_parts in GRID:
        case = (n_slots, keep, plane_images, compact_images, run_parts, compact_parts)
        p = images.plan(n_slots, ne, keep, plane_images=plane_images, compact_images=compact_images, run_parts=run_parts,
                        compact_parts=compact_parts)
        planes = bool(keep and plane_images)
        compact = bool(planes and compact_images)
        layout = NONE if not keep else COMPACT if compact else PLANES if planes else RECORDS
        parts = _parts(n_slots, keep, compact, run_parts, compact_parts)
        assert p["layout"] == layout, case
        assert p["n_slots"] == n_slots, case
        assert p["elems"] == ((N_FIELDS + ne) * n_slots if keep else 0), case
        assert p["parts"] == parts, case
        assert p["fetch_parts"] == (1 if compact else parts), case
        assert p["halves"] == (2 if parts > 1 else 1), case
        assert p["begin"] == [_part_begin(n_slots, parts, k) for k in range(parts + 1)], case
        if compact:
            assert (p["blk_shift"], p["blocks"]) == (16, (n_slots + 65535) // 65536), case
        seen.add((layout, parts))
    # the grid reaches every layout, single launches, the clamp to n_slots / 65536 and the most parts there are
    assert {l for l, _ in seen} == {NONE, RECORDS, PLANES, COMPACT}
    assert {(RECORDS, 1), (RECORDS, 16), (PLANES, 5), (COMPACT, 1), (COMPACT, 3)} <= seen


def test_plan_images_properties(images):
    for n_slots, keep, (plane_images, compact_images), run_parts, compact_parts in GRID:
        case = (n_slots, keep, plane_images, compact_images, run_parts, compact_parts)
        p = images.plan(n_slots, 1, keep, plane_images=plane_images, compact_images=compact_images, run_parts=run_parts,
                        compact_parts=compact_parts)
        b, parts = p["begin"], p["parts"]
        assert len(b) == parts + 1 and b[0] == 0 and b[-1] == n_slots, case
        assert all(x < y for x, y in zip(b, b[1:])), case
        assert 1 <= parts <= max(1, n_slots // 65536), case
        if p["layout"] == COMPACT:
            assert p["fetch_parts"] == 1, case
        assert (p["halves"] == 2) == (parts > 1), case
        if parts >= 3:
            # every bound is a real number rounded down, so a part's size is within one slot of its share: the first and the last
            # part are half a middle one to within one slot
            sizes = [y - x for x, y in zip(b, b[1:])]
            for middle in sizes[1:-1]:
                assert abs(2 * sizes[0] - middle) <= 2 and abs(2 * sizes[-1] - middle) <= 2, (case, sizes)


def test_block_shift_of_the_plan_is_the_option(images):
    for shift in (7, 8, 12, 16, 30):
        p = images.plan(70000, 1, 1, plane_images=1, compact_images=1, blk_shift=shift)
        assert (p["blk_shift"], p["blocks"]) == (shift, -(-70000 // (1 << shift)))


@pytest.mark.parametrize("ne", (1, 7, 12))
@pytest.mark.parametrize("n_total", (1, 1000))
def test_layout_resolves_to_the_offsets_of_the_kernel_arguments(images, ne, n_total):
    """A launch for slots [lo, ...) of a run of n_total slots stores field f of slot s at img[(s - lo)*img_ss + f*img_fs] and weight
    e at img_w[(s - lo)*img_ws + e], where
      planes:   img = soa + lo,       img_ss = 1,   img_fs = n_total, img_w = soa + 17*n_total + lo*ne, img_ws = ne
      records:  img = rec + lo*(17 + ne), img_ss = 17 + ne, img_fs = 1,   img_w = img + 17,             img_ws = 17 + ne
    that is: plane f of n_total doubles then the weights [slot][ne], or one record of 17 + ne doubles per slot."""
    rec = N_FIELDS + ne
    for lo in sorted({0, 1, n_total - 1} & set(range(n_total))):
        for layout in (PLANES, COMPACT):
            l = images.layout(layout, n_total, ne, lo)
            assert (l["ss"], l["fs"], l["ws"]) == (1, n_total, ne)
            assert (l["base"], l["w_base"]) == (lo, N_FIELDS * n_total + lo * ne)
        r = images.layout(RECORDS, n_total, ne, lo)
        assert (r["ss"], r["fs"], r["ws"]) == (rec, 1, rec)
        assert (r["base"], r["w_base"]) == (lo * rec, lo * rec + N_FIELDS)
        l = images.layout(PLANES, n_total, ne, lo)
        for s in sorted({lo, lo + 1, (lo + n_total) // 2, n_total - 1} & set(range(lo, n_total))):
            for f in range(N_FIELDS):
                assert l["base"] + (s - lo) * l["ss"] + f * l["fs"] == f * n_total + s
                assert r["base"] + (s - lo) * r["ss"] + f * r["fs"] == s * rec + f
            for e in range(ne):
                assert l["w_base"] + (s - lo) * l["ws"] + e == N_FIELDS * n_total + s * ne + e
                assert r["w_base"] + (s - lo) * r["ws"] + e == s * rec + N_FIELDS + e
    assert images.layout(NONE, n_total, ne, 0) == dict(ss=0, fs=0, ws=0, base=0, w_base=0)


def _cuts(b0, b1):
    """Cuts of the blocks [b0, b1) into consecutive groups: every one for up to 8 blocks; beyond, block by block, in groups of 64
    (the most the fetch copies at a time) from either end, and every cut in two."""
    n = b1 - b0
    if n <= 8:
        for mask in range(1 << (n - 1)):
            yield [b0] + [b0 + k + 1 for k in range(n - 1) if mask >> k & 1] + [b1]
        return
    yield list(range(b0, b1 + 1))
    yield list(range(b0, b1, 64)) + [b1]
    yield [b0] + list(range(b1, b0, -64))[::-1]
    for m in range(b0 + 1, b1):
        yield [b0, m, b1]


@pytest.mark.parametrize("blk_shift", (7, 12, 16))
@pytest.mark.parametrize("n_total", (1, 127, 128, 129, 70000))
def test_block_spans_tile_the_fetch(images, blk_shift, n_total):
    """the fetch of [first, first + count) follows the blocks first >> shift ... of the run group by group: whatever the groups, their
    spans are disjoint, in order, and cover exactly the positions asked for"""
    B = 1 << blk_shift
    seams = {0, n_total}
    for s in (B, 2 * B, (n_total - 1) // B * B, n_total // 2 // B * B):
        seams |= {s - 1, s, s + 1}
    seams = sorted(x for x in seams if 0 <= x <= n_total)
    blocks = (n_total + B - 1) >> blk_shift
    for first, end in itertools.combinations(seams, 2):
        count = end - first
        b0, b1 = first >> blk_shift, min(blocks, (first + count + B - 1) >> blk_shift)
        assert b0 < b1
        for cut in _cuts(b0, b1):
            at = first
            for b, e in zip(cut, cut[1:]):
                lo, hi = images.block_span(first, count, n_total, blk_shift, b, e)
                assert lo == at and lo < hi, (first, count, cut, b, e, lo, hi)
                assert max(b * B, first) == lo and hi <= min(e * B, n_total)
                at = hi
            assert at == first + count, (first, count, cut)


def test_image_planes_are_in_the_kernels_field_order(images):
    d = HipImages()
    order = [("src_start_coords", 0), ("src_start_coords", 1), ("pc_start_coords", 0), ("pc_start_coords", 1),
             ("pc_start_dir", 0), ("pc_start_dir", 1), ("pc_start_elecv", 0), ("pc_start_elecv", 1),
             ("pc_exit_coords", 0), ("pc_exit_coords", 1), ("pc_exit_coords", 2), ("pc_exit_dir", 0), ("pc_exit_dir", 1),
             ("pc_exit_elecv", 0), ("pc_exit_elecv", 1), ("pc_exit_nrefl", None), ("pc_exit_dtravel", None),
             ("exit_coord_weights", None)]
    assert len(order) == N_FIELDS + 1
    for k, (name, j) in enumerate(order):
        address = 0x1000 * (k + 1)
        if j is None:
            setattr(d, name, address)
        else:
            getattr(d, name)[j] = address
    assert images.planes(d) == [0x1000 * (k + 1) for k in range(N_FIELDS + 1)]
    # a plane the caller leaves out stays out
    d.pc_exit_nrefl = None
    d.pc_start_dir[1] = None
    got = images.planes(d)
    assert got[15] == 0 and got[5] == 0 and sum(1 for p in got if p) == N_FIELDS - 1
