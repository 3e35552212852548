"""The geometries of tests/test_gpu_resize_rows.py reach the paths of k_resize_rows they are chosen for, by the
host's launch rules restated in tests/resize_rows_cases.py (no GPU): without this a GPU comparison could pass on
inputs that never reach the code it is meant for."""
import pytest

import resize_rows_cases as R
import sweep_cases as S


def _levels(geo):
    """[(level, sizes, launch shape)] of a geometry's resized levels."""
    h, w, nlevels = geo
    sizes = R.level_sizes(h, w, nlevels)
    return [(l, sizes, R.launch_shape(sizes[l][0])) for l in range(1, nlevels)]


def test_every_geometry_is_accepted_by_the_oracle():
    for h, w, nlevels in R.ALL:
        for simd in R.SIMD_MODES + (16,):
            pyr = R.reference_pyramid(h, w, nlevels, simd)
            assert len(pyr) == nlevels and pyr[0].shape == (h, w)


def test_source_strides_cover_the_residues_and_misalignments():
    assert [w % 4 for _, w, _ in R.STRIDES] == [0, 1, 2, 3]
    for geo in R.STRIDES:
        h, w, nlevels = geo
        assert nlevels >= 3  # level 2 reads level 1 at its pitch: the hoisted alignment on a derived source
        sizes = R.level_sizes(h, w, nlevels)
        sh0 = {b["sh0"] for b in R.bands(sizes, 1)}
        # an aligned image base: a stride that is a multiple of 4 keeps every band aligned, an odd one does not
        assert (sh0 == {0}) == (w % 4 == 0), (w, sh0)
        assert len(R.bands(sizes, 1)) >= 3
    odd = [g for g in R.STRIDES if g[1] % 2]
    assert {b["sh0"] for g in odd for b in R.bands(R.level_sizes(*g), 1)} == {0, 1, 2, 3}


def test_tails_sit_where_they_are_meant_to():
    only_wave, full_wave, rem_wave, last_chunk = R.TAILS[0], R.TAILS[1], R.TAILS[2:4], R.TAILS[4]
    l, sizes, s = _levels(only_wave)[0]
    assert s["ngrp"] <= 64 and s["remw"] == 0 and not s["multi"]
    assert 0 < len(R.tail_groups(sizes, l, 32)) < s["ngrp"] and len(R.tail_groups(sizes, l, 0)) == s["ngrp"]

    l, sizes, s = _levels(full_wave)[0]
    assert s["ngrp"] > 64 and s["remw"] == 0 and s["last_chunk"] >= 40 and not s["multi"]
    tails = R.tail_groups(sizes, l, 32)
    assert tails and min(tails) >= 64 * (s["wg"] - 1)  # all in the last full wave: the others take the untailed body

    for geo, chunk in zip(rem_wave, (1, 39)):
        l, sizes, s = _levels(geo)[0]
        assert s["remw"] == 1 and s["last_chunk"] == chunk
        tails = R.tail_groups(sizes, l, 32)
        assert tails and min(tails) >= 64 * s["wg"]  # only in the remainder wave

    l, sizes, s = _levels(last_chunk)[0]
    assert sizes[l][0] > 2048 and s["multi"] and s["threads"] == 512 and s["wg"] == 9 and s["wgl"] == 8
    tails = R.tail_groups(sizes, l, 32)
    assert tails and min(tails) >= 64 * 8  # wave 0 walks chunks 0 and 8, only chunk 8 has the tail
    assert R.SIMD_MODES == (0, 32)


def test_block_sizes_and_slot_counts():
    threads = {}
    for geo in R.BLOCKS:
        for l, sizes, s in _levels(geo):
            threads.setdefault((s["threads"], s["multi"]), geo)
    assert {t for t, _ in threads} == {256, 320, 384, 448, 512}
    assert (512, True) in threads and (512, False) in threads

    def slots(geo):
        out = set()
        for l, sizes, s in _levels(geo):
            for m in range(4):
                out |= {-(-b["ndw"] // s["threads"]) for b in R.bands(sizes, l, m)}
        return out

    every = set().union(*(slots(g) for g in R.ALL))
    assert 1 in every                 # a staged run shorter than one dword per thread (see the heights)
    assert R.PASS_SLOTS in every      # a pass filled exactly
    assert max(every) > R.PASS_SLOTS  # and a second pass
    # at the smallest block too, where a slot is 256 dwords
    l, sizes, s = _levels(R.SLOTS[0])[0]
    assert s["threads"] == 256 and max(slots(R.SLOTS[0])) == R.PASS_SLOTS
    l, sizes, s = _levels(R.SLOTS[1])[0]
    assert s["threads"] == 256 and max(slots(R.SLOTS[1])) == R.PASS_SLOTS + 1
    # the thresholds between the 8-, 16- and 24-slot passes are all met
    assert any(n <= 8 for n in every) and any(8 < n <= 16 for n in every) and any(16 < n <= 24 for n in every)


def test_heights_cover_the_band_and_set_remainders():
    residues, short, odd_sets, empty_sets = set(), False, False, False
    for geo in R.HEIGHTS:
        for l, sizes, s in _levels(geo):
            residues.add(sizes[l][1] % R.BAND_ROWS)
            for b in R.bands(sizes, l):
                assert b["nrow"] <= R.BAND_ROWS
                short |= b["ndw"] < s["threads"]
                per_set = R.set_rows(b["nrow"], s["sets"])
                odd_sets |= any(n % 2 for n in per_set) and s["sets"] > 1
                empty_sets |= 0 in per_set
    assert {0, 1, R.BAND_ROWS - 1} <= residues
    assert short and odd_sets and empty_sets
    # a two-set block whose last band splits 8 + 7
    l, sizes, s = _levels(R.HEIGHTS[3])[0]
    assert s["sets"] == 2 and R.set_rows(R.bands(sizes, l)[-1]["nrow"], 2) == [8, 7]


def test_batch_geometry_and_contents():
    h, w, nlevels = R.BATCH
    assert R.BATCH in R.HEIGHTS and w % 4 and (w * h) % 4 and nlevels == S.MIXED_NLEVELS
    first, second = S.mixed_batch(h, w, 3, 7000, 1), S.mixed_batch(h, w, 3, 8000, 4)
    for a, b in zip(first.images, second.images):
        assert (a != b).any()
    # results that depend on the resized levels: keypoints above level 0 in the replaced batch
    assert any(r.levels_with_keypoints() - {0} for r in second.image_refs)
    assert any((r.status == 1).any() for r in second.pair_refs)
