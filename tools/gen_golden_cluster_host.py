"""Fixture tests/golden/cluster_host_ws.json for tests/test_cluster_host.py: the workspace sizes the cluster / similarity
entries report over the test's table, recorded from the library CENTERCLIP_HIP_LIB names - the build of the commit in front
of a host-path change.  The variable is required: recorded from the tree's own build the fixture would compare the library
with itself.  Needs no GPU.

    CENTERCLIP_HIP_LIB=/path/to/parent/libcenterclip_hip.so python tools/gen_golden_cluster_host.py
"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centerclip_amd import _lib as L                             # noqa: E402


def _test_module():
    """tests/test_cluster_host.py, loaded by path (tests/ is no package): it owns the table and the file's name"""
    spec = importlib.util.spec_from_file_location("test_cluster_host", os.path.join(ROOT, "tests", "test_cluster_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    path = os.environ.get("CENTERCLIP_HIP_LIB")
    if not path or os.path.abspath(path) == os.path.abspath(L.LIB_PATH):
        sys.exit("set CENTERCLIP_HIP_LIB to the library of the commit the new build is compared with (not the tree's own)")
    t = _test_module()
    table = t.workspace_table(L.lib())
    with open(t.GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(t.GOLDEN, "from", path, {k: len(v) for k, v in table.items()})
