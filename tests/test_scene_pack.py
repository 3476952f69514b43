"""The scene packer (csrc/host/scene_pack.cpp: the tables the kernels read, CPU only) against digests recorded
before it moved out of the C ABI file: tools/pack_dump.cpp prints, per table of the packed scene, the element count
and the FNV-1a 64 of its bytes, and every line must equal tests/golden/scene_pack_tables.txt. No tolerance: the
tables are the product's bit-parity input (octant centres, cull padding, slot-bound codes, kd / pi), so any changed
quantisation rule, BVH split or table order shows here, by table name, before it shows as a GPU frame mismatch.

The packer's one error (RT_E_INVAL: a mesh with 2^25 or more octree leaves) needs an octree of over 33 million
leaves, so it is left to code reading; the dump's failure path is checked with the loader's message instead."""
import os
import subprocess

import pytest

from conftest import REPO, SCENES, scene_path
from test_host_prep import _speck_toml

GOLDEN = os.path.join(REPO, "tests", "golden", "scene_pack_tables.txt")


@pytest.fixture(scope="module")
def pack_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_dump") / "pack_dump")
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "raytracer-server_amd"), "pack_dump", f"PACK_DUMP={exe}"],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def golden():
    sections, name = {}, None
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("#"):
            continue
        if line.startswith("["):
            name = line.strip("[]")
            sections[name] = []
        else:
            sections[name].append(line)
    return sections


def _dump(exe, toml, assets, **env):
    e = {k: v for k, v in os.environ.items() if k != "RT_TEST_SLOT_MAX_PID"}
    e.update(env)
    out = subprocess.run([exe, toml, assets], capture_output=True, text=True, timeout=120, env=e)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _rows(lines):
    return {ln.split()[0]: ln.split()[1:] for ln in lines}


@pytest.mark.parametrize("name", ["cornell_box", "cubes", "flying_unicorn"])
def test_reference_scenes_pack_to_the_recorded_tables(name, pack_dump, golden):
    got = _dump(pack_dump, scene_path(name), os.path.join(SCENES, "assets"))
    assert len(golden[name]) == 27  # 15 tables, ctab + flag, ctab32, 3 f32 tables, off32, light_pdf, 4 traits
    assert got == golden[name]


def test_unicorn_without_slot_tables_packs_to_the_recorded_tables(pack_dump, golden):
    """RT_TEST_SLOT_MAX_PID=0 (read by pack_scene): the slot tables cleared, every other table as before."""
    got = _dump(pack_dump, scene_path("flying_unicorn"), os.path.join(SCENES, "assets"), RT_TEST_SLOT_MAX_PID="0")
    assert got == golden["flying_unicorn RT_TEST_SLOT_MAX_PID=0"]
    rows, full = _rows(got), _rows(golden["flying_unicorn"])
    for table in ("slots", "node_box", "pid_up"):
        assert rows[table][0] == "0" and full[table][0] != "0"
    assert {k: v for k, v in rows.items() if k not in ("slots", "node_box", "pid_up")} == \
           {k: v for k, v in full.items() if k not in ("slots", "node_box", "pid_up")}


def test_speck_packs_to_the_recorded_tables_without_slot_tables(pack_dump, golden, tmp_path):
    """test_host_prep's mesh smaller than its own cull padding: its bound codes clamp, so no slot tables."""
    got = _dump(pack_dump, _speck_toml(tmp_path), str(tmp_path))
    assert got == golden["speck"]
    rows = _rows(got)
    assert rows["slots"][0] == "0" and rows["node_box"][0] == "0" and rows["pid_up"][0] == "0"
    assert int(rows["mesh_nodes"][0]) > 1  # an octree with parents: there were slot rows to encode


def test_dump_fails_with_the_loaders_message(pack_dump, tmp_path):
    bad = tmp_path / "bad.toml"
    bad.write_text('[camera]\npos = [0.0, 0.0, 0.0]\ndir = [0.0, 0.0, 1.0]\n[[objects]]\nemitted = [1.0, 1.0, 1.0]\n')
    out = subprocess.run([pack_dump, str(bad), str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and out.stdout == ""
    assert "missing field `brdf`" in out.stderr
