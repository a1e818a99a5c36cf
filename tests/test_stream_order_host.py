"""The premises of stream-order tests that hold without a device: the two input variants of tests/streamcases.py have one structure, and the
oracle's tiles of A and B differ for every glyph -- so a kernel that read A where B was due cannot pass by coincidence."""
import numpy as np

import streamcases as SC


def test_the_variants_share_their_structure_and_nothing_else():
    v = SC.variants()
    a, b = v["A"], v["B"]
    assert len(a["shapes"]) == len(b["shapes"]) == 43
    for g, (s, t) in enumerate(zip(a["shapes"], b["shapes"])):
        assert (s.contour_offsets == t.contour_offsets).all() and (s.types == t.types).all() and s.inverse_y == t.inverse_y, g
        assert not np.array_equal(s.points, t.points), g
        assert sorted(bin(int(c)).count("1") for c in s.colors) == sorted(bin(int(c)).count("1") for c in t.colors), g   # (a permutation of the channels)
        assert np.allclose(np.array(s.bounds()), np.array(t.bounds()), rtol=0, atol=1e-9*max(1., float(np.abs(s.bounds()).max()))), g   # reflected in its own bounds
        assert not np.array_equal(a["xfs"][g], b["xfs"][g]) and a["xfs"][g][5] != b["xfs"][g][5], g
        assert tuple(a["sizes"][g]) != tuple(b["sizes"][g]), g
        back = SC.mirrored(t)                                                # (the variant is its own inverse)
        assert (back.colors == s.colors).all() and np.allclose(back.points, s.points, rtol=0, atol=1e-9*max(1., float(np.abs(s.points).max()))), g
    assert any((np.asarray(s.colors) != np.asarray(t.colors)).any() for s, t in zip(a["shapes"], b["shapes"]))
    assert (int(a["sizes"][:, 0].max()), int(a["sizes"][:, 1].max())) == (int(b["sizes"][:, 0].max()), int(b["sizes"][:, 1].max())) == (SC.W, SC.H)   # one slot
    oa, _, na = SC.rectangles("A", 43, 3)
    ob, _, nb = SC.rectangles("B", 43, 3)
    assert na == nb and (oa != ob).all() and int(ob.max())+SC.W*SC.H*3 <= nb and int(ob.min()) >= 0
    r = SC.repeated("B", 6)
    assert len(r["shapes"]) == 258 and r["shapes"][43+5] is b["shapes"][5]


def test_the_oracles_tiles_of_a_and_b_differ_for_every_glyph(oracle):
    v = SC.variants()
    for mode in (3, 4):
        tiles, stencils = {}, {}
        for k in "AB":
            stencils[k] = np.zeros((43, SC.H, SC.W), np.uint8)
            tiles[k] = np.stack([oracle.generate(s, mode, SC.W, SC.H, xf, stencil=stencils[k][g]) for g, (s, xf) in enumerate(zip(v[k]["shapes"], v[k]["xfs"]))])
        assert SC.equal_glyphs(tiles["A"], tiles["B"], 43) == [], mode
        same = SC.equal_glyphs(stencils["A"], stencils["B"], 43)             # (the stencil: only glyphs whose stencil is ONE value throughout, three
        assert len(same) <= 3 and all(np.unique(stencils["B"][g]).size == 1 for g in same), (mode, same)   # one-contour glyphs, may share it between A and B)
        swapped = np.stack([oracle.generate(s, mode, SC.W, SC.H, xf) for s, xf in zip(v["A"]["shapes"], v["B"]["xfs"])])   # the transform alone (the wrapper tests)
        assert SC.equal_glyphs(tiles["A"], swapped, 43) == [], mode


def test_verdict_names_stale_bytes():
    a, b = np.arange(8, dtype=np.float32), np.arange(8, dtype=np.float32)
    assert SC.verdict("x", a, b) is None
    b[3] = 9
    msg = SC.verdict("x", a, b, stale=a)
    assert "differ" in msg and "other variant" in msg and SC.equal_glyphs(a, b, 4) == [0, 2, 3]
