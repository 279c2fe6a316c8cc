"""What tests/test_gpu_ref16_limit.py assumes about the scenes of tests/ref16_limit_inputs.py, settled without a GPU: the sizes straddle the 16-bit pool form's limit
as layout.h states it, the host front builds every scene byte for byte as the oracle does, and the oracle's primary rays really do reach what the scenes are there
for — leaf slots and node pairs on both sides of index 8 192 (bit 13 of a 16-bit reference), the last leaf slot and the last pair of the tree, a leaf of 64
triangles above slot 8 192, a leaf that straddles slots 8 191 | 8 192 (where `cur + 1` carries into bit 13), every BLAS of the two-level scene.  The re-leafed
description — T - 1 node pairs, the most a scene of T triangles can have — is held to the built tree it came from: the same triangles in the same slots, the same
nearest hits from a float32 restatement of the reference's walk over it, and the oracle's hits themselves to a float64 brute force over every triangle."""
import numpy as np
import pytest

import bvh_build_inputs as B
import mesh_truth as mt
import ref16_limit_inputs as I
import stack_fill as S
from conftest import ASSETS

W, H = I.W, I.H
FILE_SCENES = {"file_narrow": lambda: I.file_mesh(I.T_NARROW), "file_wide": lambda: I.file_mesh(I.T_WIDE), "big_leaf": I.big_leaf_mesh}
TWO_LEVEL = {"two_narrow": I.T_NARROW, "two_wide": I.T_WIDE}
TOTAL = {"file_narrow": I.T_NARROW, "file_wide": I.T_WIDE, "big_leaf": I.T_NARROW, "two_narrow": I.T_NARROW, "two_wide": I.T_WIDE}
NARROW = ("file_narrow", "big_leaf", "two_narrow")


class Case:
    """a scene on the oracle: its BVHs, their uploaded layout, and the default camera's primary hits with the global leaf slot and the highest pair of each mesh hit"""

    def __init__(self, orc, name, tmp):
        self.name = name
        if name in FILE_SCENES:
            self.kind, self.xml = 0, None
            self.p = FILE_SCENES[name]()
            self.o = S.mesh_oracle(orc, self.p)
        else:
            self.kind, self.xml = 1, I.write_two_level(tmp, TWO_LEVEL[name])
            self.o, _ = orc.load_scene(self.xml, 1, ASSETS)
        self.o.renderer_init(W, H)
        self.bvhs = [self.o.bvh(i) for i in range(self.o.bvh_count())]
        self.layout = I.Layout(self.bvhs)
        self.hits, self.O, self.D = I.primary_hits(self.o)
        self.mesh, self.blas, self.slot, self.high = self.resolve(self.hits)

    def resolve(self, hits):
        """(mask of the mesh hits, their BVH, global leaf slot, highest pair on the path to their leaf)"""
        mesh = hits["objIdx"] >= 2
        blas = (hits["objIdx"][mesh] - 2) if self.kind == 1 else np.zeros(int(mesh.sum()), np.int64)
        return mesh, blas, self.layout.slots(blas, hits["triIdx"][mesh]), self.layout.highest_pair(blas, hits["triIdx"][mesh])


@pytest.fixture(scope="module")
def cases(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ref16_limit"); made = {}

    def get(name):
        if name not in made:
            made[name] = Case(orc, name, tmp)
        return made[name]
    return get


# 1. the sizes are the rule's, and the rule is the header's
def test_sizes_straddle_the_limit_the_header_states():
    assert (I.REF16_MAX_INDEX, I.REF16_INDEX_MASK, I.BIT13) == (0x3ffe, 0x3fff, 8192)
    assert I.T_NARROW == I.REF16_MAX_INDEX and I.T_WIDE == I.T_NARROW + 1
    # the highest index a scene of T triangles puts into a reference is the last triangle's, slot + 1 = T: it fits the mask with the tag bits clear up to T_NARROW, and
    # the node pairs of T triangles are at most T - 1
    assert I.T_NARROW & ~I.REF16_INDEX_MASK == 0 and I.T_NARROW <= I.REF16_MAX_INDEX < I.T_WIDE
    assert sum(I.piece_sizes(I.T_NARROW)) == I.T_NARROW and sum(I.piece_sizes(I.T_WIDE)) == I.T_WIDE
    assert I.piece_sizes(I.T_NARROW)[:2] == I.piece_sizes(I.T_WIDE)[:2] == (5000, 5000)


# 2. per scene: the totals, and the host front's build against the oracle's
@pytest.mark.parametrize("name", list(TOTAL))
def test_host_front_builds_the_scenes_as_the_oracle_does(crt, cases, name):
    c = cases(name)
    assert sum(len(b["tris"]) for b in c.bvhs) == c.layout.tris == TOTAL[name]
    assert c.layout.pairs <= I.REF16_MAX_INDEX
    if c.kind == 0:
        assert I.positions(c.bvhs[0]).tobytes() == c.p.tobytes()
        t = crt.host_bvh_build(c.p); b = c.bvhs[0]
        B.assert_bvh_equal(t, dict(nodes=b["nodes"][:b["nodesUsed"]], indices=b["triIndices"], nodesUsed=b["nodesUsed"], maxDepth=b["maxDepth"]), name)
        return
    hs = crt.HostScene(c.xml, 1, ASSETS)
    sizes = I.piece_sizes(TOTAL[name])
    assert hs.bvh_count() == len(c.bvhs) == 3
    for i, n in enumerate(sizes):
        a, b = hs.bvh(i), c.bvhs[i]
        assert len(a["tris"]) == len(b["tris"]) == n
        assert I.positions(b).tobytes() == I.piece(i, n).tobytes()                # the OBJ text holds the generated coordinates exactly
        assert a["nodesUsed"] == b["nodesUsed"] and a["maxDepth"] == b["maxDepth"]
        assert a["nodes"].tobytes() == b["nodes"].tobytes() and np.array_equal(a["triIndices"], b["triIndices"])
        assert a["tris"].tobytes() == b["tris"].tobytes()
    assert hs.tlas()[0].tobytes() == c.o.tlas()[0].tobytes()
    assert c.layout.tri_base == [0, 5000, 10000]                            # BLAS 2's triangles occupy global slots 10 000 .. total - 1


# 3. the default camera's primary rays reach both halves of the index range, by leaf slot and by node pair
@pytest.mark.parametrize("name", list(TOTAL))
def test_default_camera_hits_leaves_and_pairs_on_both_sides_of_bit_13(cases, name):
    c = cases(name)
    seen = dict(mesh=int(c.mesh.sum()), high=int((c.slot >= I.BIT13).sum()), low=int((c.slot < I.BIT13).sum()), pairs_high=int((c.high >= I.BIT13).sum()),
                top_slot=int(c.slot.max()), per_blas=np.bincount(c.blas, minlength=len(c.bvhs)).tolist())
    print(name, seen)
    assert seen["high"] >= 200 and seen["low"] >= 100, seen
    assert seen["pairs_high"] >= 100, seen
    if c.kind == 1:
        assert min(seen["per_blas"]) >= 100, seen
    # the helpers agree with each other: the highest pair of a path is its last, and the path's pairs rise
    b, tri = int(c.blas[0]), int(c.hits["triIdx"][c.mesh][0])
    path = c.layout.pairs_to(b, tri)
    assert path == sorted(path) and path[-1] == c.high[0] and len(path) <= c.bvhs[b]["maxDepth"] + 1


# 4. the second camera looks at the triangle in the last leaf slot, whose reference is the form's last index
def test_second_camera_hits_the_last_leaf_slot_and_the_last_pair(orc, cases):
    c = cases("file_narrow"); L = c.layout
    assert int(c.slot.max()) < I.T_NARROW - 1                               # the default camera does not reach it: hence this one
    _, tri = L.triangle_in_slot(I.T_NARROW - 1)
    assert L.slots(0, tri) == I.T_NARROW - 1 and L.slots(0, tri) + 1 == I.REF16_MAX_INDEX
    pos, target = I.close_camera(c.p, tri)
    o = S.mesh_oracle(orc, c.p); o.renderer_init(W, H)                      # (an oracle of its own: the shared one keeps the default camera)
    o.set_camera_state(pos, target)
    hits, _, _ = I.primary_hits(o)
    mesh, blas, slot, high = c.resolve(hits)
    on_it = int((slot == I.T_NARROW - 1).sum())
    print("pixels on the last slot's triangle", on_it, "mesh hits", int(mesh.sum()), "paths through the last pair", int((high == L.pairs - 1).sum()))
    assert on_it >= 4
    assert (high == L.pairs - 1).any()                                      # the last pair of the tree lies on a hit path
    assert L.pairs_to(0, tri)[-1] <= L.pairs - 1


# 5. the big leaf
def test_big_leaf_lies_above_bit_13_and_is_seen(cases):
    c = cases("big_leaf")
    nodes = c.bvhs[0]["nodes"][:c.bvhs[0]["nodesUsed"]]
    big = int(np.argmax(nodes["triCount"]))
    first, count = int(nodes["leftFirst"][big]), int(nodes["triCount"][big])
    assert count >= 64 and count == I.BIG_LEAF and first > I.BIT13, (first, count)
    copies = np.sort(c.bvhs[0]["triIndices"][first:first + count])
    assert np.array_equal(copies, np.arange(I.T_NARROW - I.BIG_LEAF, I.T_NARROW))      # the leaf is the copies, all of them
    assert (I.positions(c.bvhs[0])[copies] == I.BIG_TRIANGLE).all()
    inside = (c.slot >= first) & (c.slot < first + count)
    print("primary rays on the big leaf", int(inside.sum()))
    assert inside.sum() >= 50
    assert (c.slot[inside] == first).all()                                  # tied hits go to the leaf's first slot: the walk keeps the first of equal t


# 6. a leaf of >= 2 triangles straddles slots 8 191 | 8 192 in every narrow scene
@pytest.mark.parametrize("name", NARROW)
def test_a_leaf_straddles_the_carry_into_bit_13(cases, name):
    c = cases(name)
    leaf = c.layout.leaf_across(I.BIT13)
    assert leaf is not None, "no leaf holds slots %d and %d: choose another seed" % (I.BIT13 - 1, I.BIT13)
    b, node, first, count = leaf
    assert count >= 2 and first <= I.BIT13 - 1 and first + count > I.BIT13
    if c.kind == 1:
        assert b == 1                                                       # BLAS 1 holds global slots 5 000 .. 9 999


# 7. the rebuilds of the scene-write test change BLAS 0's pair count, so the later BLASes' pairs move
def test_rebuilt_blas_0_has_another_pair_count(crt, cases):
    c = cases("two_narrow")
    own = crt.host_bvh_build(I.piece(0, I.PIECE_TRIS)); moved = crt.host_bvh_build(I.wobbled_piece0())
    assert own["nodesUsed"] == c.bvhs[0]["nodesUsed"]
    delta = moved["nodesUsed"] // 2 - own["nodesUsed"] // 2
    print("pairs of BLAS 0", own["nodesUsed"] // 2, "->", moved["nodesUsed"] // 2, "pair bases", c.layout.pair_base)
    assert delta != 0
    assert c.layout.pairs + delta <= I.REF16_MAX_INDEX                      # still a narrow scene
    assert c.layout.pairs > I.BIT13 and c.layout.pairs + delta > I.BIT13     # the moved references lie round and above index 8 192 either way
    assert c.layout.pair_base[2] < I.BIT13 < c.layout.pairs


# 8. the re-leafed description
def test_releafed_description_keeps_every_triangle_in_its_slot(crt, orc, cases):
    c = cases("file_narrow")
    t = crt.host_bvh_build(c.p); r = I.releaf(t, c.p)
    nodes = r["nodes"]
    assert r["nodesUsed"] == len(nodes) == 2 * I.T_NARROW - 1 and r["nodesUsed"] // 2 == I.T_NARROW - 1 == 16381
    leaves = nodes["triCount"] > 0
    assert (nodes["triCount"][leaves] == 1).all() and leaves.sum() == I.T_NARROW
    assert np.array_equal(np.sort(nodes["leftFirst"][leaves]), np.arange(I.T_NARROW))        # every slot in exactly one leaf
    assert np.array_equal(r["indices"], t["indices"]) and np.array_equal(r["indices"], c.bvhs[0]["triIndices"])
    inner = np.flatnonzero(~leaves)
    assert (nodes["leftFirst"][inner] & 1).all() and (nodes["leftFirst"][inner] > inner).all()      # pairwise at an odd index, behind the parent
    assert np.array_equal(np.sort(np.concatenate([nodes["leftFirst"][inner], nodes["leftFirst"][inner] + 1])), np.arange(1, len(nodes)))
    old = t["nodes"][:t["nodesUsed"]]
    assert nodes["aabbMin"][:len(old)].tobytes() == old["aabbMin"].tobytes() and nodes["aabbMax"][:len(old)].tobytes() == old["aabbMax"].tobytes()
    par = I.parents(nodes)                                                  # a child's box lies inside its parent's
    assert (nodes["aabbMin"][1:] >= nodes["aabbMin"][par[1:]]).all() and (nodes["aabbMax"][1:] <= nodes["aabbMax"][par[1:]]).all()
    lo, hi = c.p.min(axis=1), c.p.max(axis=1)
    li = np.flatnonzero(leaves); tri = r["indices"][nodes["leftFirst"][li]]
    assert np.array_equal(nodes["aabbMin"][li], lo[tri]) and np.array_equal(nodes["aabbMax"][li], hi[tri])   # every leaf's box is its triangle's own
    assert r["added_levels"] == 1 and r["height"] == t["height"] + 1 == B.depths(nodes).max()       # one more stack level
    # the last pair index, 16 380, lies on the path to the triangle in the last leaf slot: the one the second camera looks at and hits (test 4)
    assert I.pair_of_node(len(nodes) - 1) == I.T_NARROW - 2 == 16380
    rl = I.Layout([dict(nodes=nodes, nodesUsed=r["nodesUsed"], indices=r["indices"])])
    assert rl.pairs == I.T_NARROW - 1 and np.array_equal(rl.slot[0], c.layout.slot[0])
    last = int(r["indices"][-1])
    assert rl.pairs_to(0, last)[-1] == 16380 and rl.pairs_to(0, last)[:-1] == c.layout.pairs_to(0, last)
    # a float32 restatement of the reference's walk over the re-leafed tree finds the oracle's hits: t, u, v, object and triangle, bit for bit
    world = S.World(orc, c.o)
    world.parts[0] = S.Bvh(dict(nodes=nodes, triIndices=r["indices"], tris=c.bvhs[0]["tris"], nodesUsed=r["nodesUsed"]))
    assert world.parts[0].height == r["height"]
    got, _ = world.find_nearest_many(c.O, c.D, orc.HIT_DTYPE)
    for f in ("t", "u", "v", "objIdx", "triIdx"):
        assert np.array_equal(np.asarray(got[f]).view(np.uint32), np.asarray(c.hits[f]).view(np.uint32)), f


def test_oracle_hits_agree_with_a_float64_brute_force(cases):
    """every mesh hit of the default camera and every eighth other primary ray, against mesh_truth's nearest hit over all 16 382 triangles"""
    c = cases("file_narrow")
    sel = np.sort(np.concatenate([np.flatnonzero(c.mesh), np.flatnonzero(~c.mesh)[::8]]))
    with np.errstate(invalid="ignore"):
        tr = mt.nearest_truth(mt.mesh_world(c.p), c.O[sel], c.D[sel])
        viol = mt.nearest_violations(tr, c.hits[sel])
    assert not viol, {k: sel[v][:8].tolist() for k, v in viol.items()}
    assert (tr["kind_hi"] == 2).sum() >= 0.95 * c.mesh.sum() and tr["uninformative"].sum() <= 0.02 * len(sel)
