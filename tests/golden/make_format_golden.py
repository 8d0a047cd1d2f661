"""Generates the file-format fixtures of tests/test_formats.py from the reference's own serializer (oracle/_ref/interface_probe,
built by `make -C oracle ref` where the reference is present): the scene the probe writes, our writer's scene and the probe's
dump of it, and the probe's header sizes.  Run from the repo root: python tests/golden/make_format_golden.py"""
import os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
from test_formats import PROBE, write_our_scene
subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
if not os.path.exists(PROBE):
    sys.exit("the probe was not built: the reference is not present")
subprocess.check_call([PROBE, "write", os.path.join(HERE, "interface_probe_write_3_4.mvs"), "3", "4"])
ours = os.path.join(HERE, "interface_probe_ours.mvs")
write_our_scene(ours)
with open(os.path.join(HERE, "interface_probe_ours_dump.txt"), "wb") as f:
    f.write(subprocess.check_output([PROBE, "dump", ours]))
with open(os.path.join(HERE, "interface_probe_sizes.txt"), "wb") as f:
    f.write(subprocess.check_output([PROBE, "sizes"]))
print("written")
