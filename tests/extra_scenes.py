"""Scene texts shared by tests that need more than the three reference scenes (written to a directory of the
caller's choosing with `write`): tests/test_gpu_parity.py's quirk scene and the scenes of tests/vertex_states.py."""
import os

# A triangle-mesh emitter (the first emitting object is the light, scene.rs:129-137; its kd is 0), two Phong
# objects with an even power, a mirror and a diffuse prism: tests/test_gpu_parity.py
# test_phong_and_mesh_light_parity, and the vertex batteries' mesh-light scene.
QUIRK_SCENE = """
[camera]
pos = [0.0, 6.0, 60.0]
dir = [0.0, -0.1, -1.0]
[[objects]]
emitted = [12.0, 12.0, 12.0]
brdf = { type = "diffuse", kd = [0.0, 0.0, 0.0] }
geometry = { type = "cube", pos = [6.0, 14.0, -4.0], size = 4.0 }
transforms = [ { rotate_y = 0.3 } ]
[[objects]]
brdf = { type = "phong", kd = 0.5, ks = 0.3, power = 8, color_d = [0.7, 0.6, 0.5], color_s = [1.0, 1.0, 1.0] }
geometry = { type = "plane", pos = [0.0, -5.0, 0.0], n = [0.0, 1.0, 0.0] }
[[objects]]
brdf = { type = "diffuse", kd = [0.6, 0.6, 0.75] }
geometry = { type = "plane", pos = [0.0, 0.0, -30.0], n = [0.0, 0.0, 1.0] }
[[objects]]
brdf = { type = "phong", kd = 0.2, ks = 0.7, power = 24, color_d = [0.9, 0.3, 0.3], color_s = [1.0, 1.0, 1.0] }
geometry = { type = "sphere", pos = [-8.0, 0.0, 2.0], r = 5.0 }
[[objects]]
brdf = { type = "specular", ks = [0.95, 0.95, 0.95] }
geometry = { type = "sphere", pos = [9.0, -1.0, 6.0], r = 4.0 }
[[objects]]
brdf = { type = "diffuse", kd = [0.8, 0.8, 0.8] }
geometry = { type = "prism", pos = [-2.0, -5.0, -12.0], size = [6.0, 9.0, 5.0] }
"""

# A closed room under a sphere light with Phong objects of an even and an odd power (kd + ks < 1: all three
# branches of the lobe choice, absorption included), two mirrors facing each other (mirror-to-mirror chains, a
# mirror that sees the light), a wall with kd = 0 that emits nothing (behind the camera), and diffuse walls.
# Four spheres and two planes per axis: the scene fits the device's compact tables.
PHONG_SCENE = """
[camera]
pos = [50.0, 40.0, 190.0]
dir = [0.0, -0.1, -1.0]
[[objects]]
brdf = { type = "diffuse", kd = [0.75, 0.25, 0.25] }
geometry = { type = "plane", pos = [1.0, 0.0, 0.0], n = [-1.0, 0.0, 0.0] }
[[objects]]
brdf = { type = "diffuse", kd = [0.25, 0.25, 0.75] }
geometry = { type = "plane", pos = [99.0, 0.0, 0.0], n = [-1.0, 0.0, 0.0] }
[[objects]]
brdf = { type = "diffuse", kd = [0.75, 0.75, 0.75] }
geometry = { type = "plane", pos = [0.0, 0.0, 0.0], n = [0.0, 0.0, -1.0] }
[[objects]]
brdf = { type = "phong", kd = 0.5, ks = 0.3, power = 8, color_d = [0.7, 0.6, 0.5], color_s = [1.0, 1.0, 1.0] }
geometry = { type = "plane", pos = [0.0, 0.0, 0.0], n = [0.0, 1.0, 0.0] }
[[objects]]
brdf = { type = "diffuse", kd = [0.75, 0.75, 0.75] }
geometry = { type = "plane", pos = [0.0, 81.6, 0.0], n = [0.0, -1.0, 0.0] }
[[objects]]
brdf = { type = "diffuse", kd = [0.0, 0.0, 0.0] }
geometry = { type = "plane", pos = [0.0, 0.0, 200.0], n = [0.0, 0.0, 1.0] }
[[objects]]
brdf = { type = "phong", kd = 0.2, ks = 0.7, power = 25, color_d = [0.9, 0.3, 0.3], color_s = [1.0, 1.0, 1.0] }
geometry = { type = "sphere", pos = [25.0, 14.0, 60.0], r = 14.0 }
[[objects]]
brdf = { type = "specular", ks = [0.95, 0.95, 0.95] }
geometry = { type = "sphere", pos = [68.0, 18.0, 70.0], r = 18.0 }
[[objects]]
brdf = { type = "specular", ks = [0.9, 0.9, 0.99] }
geometry = { type = "sphere", pos = [40.0, 20.0, 110.0], r = 16.0 }
[[objects]]
emitted = [40.0, 40.0, 40.0]
brdf = { type = "diffuse", kd = [0.0, 0.0, 0.0] }
geometry = { type = "sphere", pos = [50.0, 68.0, 90.0], r = 5.0 }
"""

TEXTS = {"quirks": QUIRK_SCENE, "phong_room": PHONG_SCENE}


def write(directory, name):
    """Writes scene `name` of TEXTS into `directory` and returns the file's path."""
    p = os.path.join(str(directory), f"{name}.toml")
    with open(p, "w") as f:
        f.write(TEXTS[name])
    return p
