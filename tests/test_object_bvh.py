"""The object BVH on the host (csrc/host/scene_pack.cpp build_object_bvh; no GPU): the tree that
rt_scene_object_bvh reports for the scenes of tests/many_spheres.py, and the scenes that must not get one."""
import numpy as np
import pytest
import tomli

import many_spheres
from conftest import scene_path

BVH_MAX_DEPTH = 20  # scene_layout.h kBvhMaxDepth
NAMES = ["crowd", "crowd_out", "s5", "s1p17", "s4p13", "mixed", "field64"]


@pytest.fixture(scope="module")
def scenes(rt, tmp_path_factory):
    d = tmp_path_factory.mktemp("many_spheres")
    out = {}
    for n in NAMES:
        p = many_spheres.write(d, n)
        with open(p, "rb") as f:
            out[n] = (rt.Scene.from_toml(p), tomli.load(f)["objects"])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_tree_shape(scenes, name):
    sc, objs = scenes[name]
    t = sc.object_bvh()
    spheres = [i for i, o in enumerate(objs) if o["geometry"]["type"] == "sphere"]
    others = [i for i, o in enumerate(objs) if o["geometry"]["type"] != "sphere"]
    assert t is not None and len(t["a"]) > 0 and len(t["refs"]) == len(spheres)
    assert list(t["rest"]) == others  # planes and meshes, scene order
    assert sorted(t["refs"]) == spheres  # every sphere in exactly one leaf
    n, seen, max_depth = len(t["a"]), np.zeros(len(t["refs"]), dtype=int), 0

    def walk(i, depth):  # returns the index after node i's subtree (DFS pre-order: the left child is the next node)
        nonlocal max_depth
        box = t["boxes"][i]
        if t["count"][i] > 0:
            max_depth = max(max_depth, depth)
            a, c = int(t["a"][i]), int(t["count"][i])
            assert 1 <= c <= 4 or depth == BVH_MAX_DEPTH - 1
            run = t["refs"][a:a + c]
            assert np.all(np.diff(run) > 0)  # ascending within the leaf
            seen[a:a + c] += 1
            for idx in run:
                g = objs[idx]["geometry"]
                pos, r = np.array(g["pos"], dtype=float), float(g["r"])
                assert np.all(box[:3] <= pos - r) and np.all(box[3:] >= pos + r)
            return i + 1
        assert t["axis"][i] in (0, 1, 2)
        left = i + 1
        right = walk(left, depth + 1)
        assert right == t["a"][i]  # `a` is the right child, right after the left subtree
        end = walk(right, depth + 1)
        for child in (left, right):
            cb = t["boxes"][child]
            assert np.all(box[:3] <= cb[:3]) and np.all(box[3:] >= cb[3:])
        return end

    assert walk(0, 0) == n  # the nodes are exactly one tree
    assert np.all(seen == 1)
    assert max_depth == t["depth"] < BVH_MAX_DEPTH


def test_smallest_trees(scenes):
    five = scenes["s5"][0].object_bvh()
    assert len(five["a"]) == 3 and five["count"][0] == 0 and five["count"][1] + five["count"][2] == 5  # two leaves
    assert len(five["rest"]) == 0
    one = scenes["s1p17"][0].object_bvh()
    assert len(one["a"]) == 1 and one["count"][0] == 1 and len(one["rest"]) == 17 and one["depth"] == 0
    four = scenes["s4p13"][0].object_bvh()
    assert len(four["a"]) == 1 and four["count"][0] == 4 and len(four["rest"]) == 13


def test_views_answer_for_their_base(scenes):
    sc = scenes["mixed"][0]
    v = sc.view(pos=(1.0, 2.0, 30.0), dir=(0.0, 0.0, -1.0))
    a, b = sc.object_bvh(), v.object_bvh()
    assert v.info() == sc.info() and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["cornell_box", "cubes", "flying_unicorn"])
def test_reference_scenes_have_no_object_bvh(rt, name):
    sc = rt.Scene.from_toml(scene_path(name))
    assert sc.object_bvh() is None


def test_compact_scenes_have_no_object_bvh(rt, tmp_path):
    import extra_scenes

    for name in extra_scenes.TEXTS:  # the quirk scene and the Phong room: both fit the compact tables
        sc = rt.Scene.from_toml(extra_scenes.write(tmp_path, name))
        assert sc.object_bvh() is None
    # four spheres and a plane fit; a fifth sphere does not
    t = many_spheres.camera((0, 0, 20), (0, 0, -1)) + many_spheres.plane((0, -3, 0), (0, 1, 0)) + \
        many_spheres.light((0, 9, 0), 2.0)
    for k in range(3):
        t += many_spheres.sphere((3.0 * k - 3, 0, 0), 1.0)
    p = tmp_path / "four.toml"
    p.write_text(t)
    assert rt.Scene.from_toml(str(p)).object_bvh() is None
    p.write_text(t + many_spheres.sphere((0, 3, 0), 1.0))
    assert rt.Scene.from_toml(str(p)).object_bvh() is not None


def test_scene_without_spheres_has_no_object_bvh(rt, tmp_path):
    t = many_spheres.camera((0, 4, 30), (0, 0, -1))
    t += many_spheres._obj(many_spheres._DIFFUSE.format(0.0, 0.0, 0.0),
                           '{ type = "cube", pos = [0.0, 12.0, 0.0], size = 3.0 }', (9.0, 9.0, 9.0))
    for k in range(17):
        t += many_spheres.plane((0.0, -3.0 - k, 0.0), (0.0, 1.0, 0.0))
    p = tmp_path / "planes.toml"
    p.write_text(t)
    sc = rt.Scene.from_toml(str(p))
    assert sc.info()["objects"] == 18 and sc.object_bvh() is None


def test_non_finite_sphere_has_no_object_bvh(rt):
    objs = [dict(geom_kind=0, pos=[3.0 * k, 0.0, 0.0], r=1.0, brdf_kind=0, k=[0.5, 0.5, 0.5]) for k in range(5)]
    objs[0]["emitted"] = [9.0, 9.0, 9.0]
    assert rt.Scene.from_desc([0.0, 0.0, 20.0], [0.0, 0.0, -1.0], objs).object_bvh() is not None
    for bad in (dict(r=float("nan")), dict(r=float("inf")), dict(pos=[0.0, float("nan"), 0.0])):
        objs[3] = dict(objs[3], **bad)
        assert rt.Scene.from_desc([0.0, 0.0, 20.0], [0.0, 0.0, -1.0], objs).object_bvh() is None
