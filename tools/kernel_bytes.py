#!/usr/bin/env python3
"""Per-kernel hashes of the gfx950 machine code of pmoe_amd/csrc/*.hip, to show that a host-side change left every kernel alone.

    python tools/kernel_bytes.py OUT.json [CSRC_DIR]         hash the kernels of CSRC_DIR (default: this tree's pmoe_amd/csrc)
    python tools/kernel_bytes.py --compare BEFORE.json AFTER.json

Each file is compiled device-only with a fixed compilation-unit id (the id seeds the names of internal symbols), the code object
is unbundled, and every FUNC symbol's bytes of .text and every kernel descriptor (<kernel>.kd: register counts, LDS, scratch;
without its code-offset field, which moves when another kernel of the file goes) are hashed under the symbol's name.  Names and
hashes only: no instruction is inspected."""
import hashlib
import json
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROCM = Path("/opt/rocm")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "--offload-device-only"]


def hashes(src, tmp):
    obj, elf = tmp / (src.stem + ".o"), tmp / (src.stem + ".elf")
    subprocess.check_call([str(ROCM / "bin/hipcc"), *FLAGS, f"-cuid=pmoe_{src.stem}", "-c", src.name, "-o", str(obj)], cwd=src.parent)
    subprocess.check_call([str(ROCM / "lib/llvm/bin/clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}",
                           "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"])
    data = elf.read_bytes()
    readelf = str(ROCM / "lib/llvm/bin/llvm-readelf")
    sections = {}                                               # index -> (address, file offset)
    for line in subprocess.check_output([readelf, "-S", "-W", str(elf)], text=True).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[2] in ("PROGBITS", "NOBITS"):
            sections[int(f[0])] = (int(f[3], 16), int(f[4], 16))
    out = {}
    for line in subprocess.check_output([readelf, "-s", "-W", str(elf)], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[6].isdigit() and (f[3] == "FUNC" or f[7].endswith(".kd")):
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            body = bytearray(data[start:start + int(f[2])])
            if f[7].endswith(".kd"):
                body[16:24] = bytes(8)      # kernel_code_entry_byte_offset: where the code lies relative to the descriptor
            out[f[7]] = hashlib.sha256(body).hexdigest()[:16]
    return out


def main(argv):
    if argv[0] == "--compare":
        before, after = (json.loads(Path(p).read_text()) for p in argv[1:3])
        bad = 0
        print(f"{'file':14} {'kernels':>7} {'same':>5} {'differ':>6}  only before")
        for name in sorted(before):
            b, a = before[name], after.get(name, {})
            differ = sorted(k for k in b if k in a and a[k] != b[k])
            gone, new = sorted(k for k in b if k not in a and not k.endswith(".kd")), sorted(set(a) - set(b))
            bad += len(differ) + len(new)
            print(f"{name:14} {sum(not k.endswith('.kd') for k in b):7} {sum(k in a and a[k] == b[k] and not k.endswith('.kd') for k in b):5} "
                  f"{len(differ):6}  {' '.join(gone) or '-'}" + (f"  NEW: {' '.join(new)}" if new else ""))
            for k in differ:
                print("   differs:", k)
        return 1 if bad else 0
    csrc = Path(argv[1]) if len(argv) > 1 else Path(__file__).resolve().parents[1] / "pmoe_amd" / "csrc"
    srcs = sorted(csrc.glob("*.hip"))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        table = dict(zip((s.name for s in srcs), pool.map(lambda s: hashes(s, Path(tmp)), srcs)))
    Path(argv[0]).write_text(json.dumps(table, indent=0, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
