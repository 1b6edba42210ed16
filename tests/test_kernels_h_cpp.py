"""The host-kernel interface (csrc/kernels.h) is declared once and both sides use it.

* ``test_kernels_h_under_host_compiler``: the header compiles under the plain host compiler, and
  ``pvr::AdamGroup`` reads the float32 [G, 10] table that ``FusedAdam._group_array`` writes
  (tests/cpp/test_kernels_h.cpp).
* ``test_launchers_declared_once``: no ``extern "C"`` prototype of a ``pvr_*`` function outside the
  header (``pvr_src_hash`` in bindings.cpp, defined by the build, is the one exception), and every
  name the header declares is defined in exactly one ``.hip`` file. A definition that disagrees with
  its declaration is then a compile error (C linkage cannot be overloaded)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_vit_paper_replication_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_kernels_h.cpp")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.skipif(not os.path.isdir(os.path.join(ROCM_INC, "hip")), reason="no ROCm headers")
def test_kernels_h_under_host_compiler(tmp_path):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    p0, p1 = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([dict(params=[p0], lr=2.0, weight_decay=0.0625, decoupled_weight_decay=True),
                     dict(params=[p1], lr=3.0, weight_decay=0.0)], betas=(0.375, 0.75), eps=0.125)
    table = opt._group_array(1)
    assert table.shape == (2, 10) and table.dtype.name == "float32"
    table.tofile(str(tmp_path / "groups.bin"))
    exe = str(tmp_path / "test_kernels_h")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INC}", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(tmp_path / "groups.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = _strip_comments(f.read())
    return out


# a pvr_* function head up to the character that ends it: ';' a prototype, '{' a definition
HEAD = re.compile(r"\b(pvr_\w+)\s*\(([^(){};]*)\)\s*([;{])")


def test_launchers_declared_once():
    srcs = _sources()
    header = srcs.pop("kernels.h")
    declared = [m.group(1) for m in HEAD.finditer(header) if m.group(3) == ";"]
    assert "pvr_gemm" in declared and "pvr_attn_bwd" in declared
    assert len(set(declared)) == len(declared), "a launcher is declared twice in kernels.h"
    assert not [m.group(1) for m in HEAD.finditer(header) if m.group(3) == "{"], "kernels.h defines a function"

    defined = {}
    for name, text in srcs.items():
        for m in re.finditer(r'extern\s+"C"\s*([^;{}]*?)\b(pvr_\w+)\s*\(([^(){};]*)\)\s*([;{])', text):
            fn, end = m.group(2), m.group(4)
            if end == ";":
                assert (name, fn) == ("bindings.cpp", "pvr_src_hash"), f'{name} re-declares extern "C" {fn}'
            else:
                defined.setdefault(fn, []).append(name)
        assert not re.search(r'extern\s+"C"\s*\{', text), f'{name} opens an extern "C" block'
        if name.endswith(".hip") or name == "bindings.cpp":
            assert '#include "kernels.h"' in text, f"{name} does not include kernels.h"
    for fn in declared:
        files = defined.get(fn, [])
        assert len(files) == 1 and files[0].endswith(".hip"), f"{fn}: defined in {files or 'no file'}"
    assert sorted(defined) == sorted(declared), "a launcher is defined without a declaration in kernels.h"
