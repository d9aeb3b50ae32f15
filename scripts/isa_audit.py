"""What the compiler made of the level-1 parser's kernels and of the record decoder, without a GPU.

    python scripts/isa_audit.py                  build the device code of the tree (hipcc, the product's flags) and audit it
    python scripts/isa_audit.py path/to/lib.so   audit the gfx950 code object inside a built library
    ... --keep DIR                               leave the code object and its disassembly in DIR

Disassembles k_l1_parse<10>, k_l1_duplex<1,1,3> and k_decode_rec (llvm-objdump) and prints, per kernel: code bytes, branch instructions, s_nops,
`v_cndmask 0,1 -> v_cmp_ne` pairs (a lane mask turned into a 0/1 vector and back into a mask: what a BALLOT of a conjunction
compiles to), `v_cndmask 0,1 -> v_readfirstlane` pairs (a wave-uniform bool that travels through a vector register), and the
registers / spills / scratch / LDS of the kernel's metadata; a build adds the occupancy of -Rpass-analysis=kernel-resource-usage.
The counts are static (instructions in the code, not executed ones) and move with the compiler: a record, not a test.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = (("k_l1_parse<10>", "10k_l1_parseILi10EE"), ("k_l1_duplex<1,1,3>", "11k_l1_duplexILi1ELi1ELi3EE"),
           ("k_decode_rec", "12k_decode_recE"))
WINDOW = 12          # instructions within which the consumer of a v_cndmask 0,1 is looked for


def llvm(tool):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return shutil.which(tool) or tool


def build_code_object(tmp):
    """Device-only compile of the product's kernels with the product's flags; returns (code object, {mangled name: occupancy})."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    co = os.path.join(tmp, "plz4hip.co")
    cmd = [hipcc, "--offload-arch=gfx950", "--offload-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-fno-slp-vectorize", "-Wno-unused-value",
           "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-c", "-o", co,
           os.path.join(ROOT, "plz4_amd", "csrc", "plz4hip.hip")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode:
        sys.exit(p.stdout)
    occ, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            occ[name] = int(m.group(1))
    return co, occ


def extract_code_object(lib, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.check_call([llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def disassemble(co):
    """{symbol: [(address, mnemonic, operands, bytes)]}"""
    out = subprocess.check_output([llvm("llvm-objdump"), "-d", co], text=True)
    if KEEP:
        with open(os.path.join(KEEP, "device.s"), "w") as f:
            f.write(out)
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)(?:<.*>)?\s*$", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2), 4 * len(m.group(4).split())))
    return funcs


def metadata(co):
    """{kernel name: {field: value}} from the code object's notes"""
    out = subprocess.check_output([llvm("llvm-readelf"), "--notes", co], text=True)
    meta, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- .agpr_count") or (line.lstrip().startswith("- ") and m.group(1) == "agpr_count"):
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name" and m.group(2).startswith("_Z"):
            meta[m.group(2)] = cur
    return meta


def audit(ins):
    n = len(ins)
    code = (ins[-1][0] + ins[-1][3] - ins[0][0]) if n else 0
    branches = sum(1 for i in ins if i[1].startswith("s_cbranch") or i[1] == "s_branch")
    nops = sum(1 for i in ins if i[1] == "s_nop")
    to_cmp = to_rfl = 0
    for k, (_, op, args, _) in enumerate(ins):
        if not op.startswith("v_cndmask_b32"):
            continue
        a = [x.strip() for x in args.split(",")]
        if len(a) < 4 or a[1] != "0" or a[2] not in ("1", "-1"):
            continue
        dst = a[0]
        for _, op2, args2, _ in ins[k + 1:k + 1 + WINDOW]:
            a2 = [x.strip() for x in args2.split(",")]
            if op2.startswith("v_cmp_ne_u32") and dst in a2[1:]:
                to_cmp += 1
                break
            if op2 == "v_readfirstlane_b32" and len(a2) > 1 and a2[1] == dst:
                to_rfl += 1
                break
            if a2 and a2[0] == dst:
                break
    kinds = {"SALU": 0, "VALU": 0, "v_readlane": 0, "LDS": 0, "VMEM": 0}
    for _, op, _, _ in ins:
        if op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane"):
            kinds["v_readlane"] += 1
        elif op.startswith("v_"):
            kinds["VALU"] += 1
        elif op.startswith("ds_"):
            kinds["LDS"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            kinds["VMEM"] += 1
        elif op.startswith("s_") and not op.startswith(("s_cbranch", "s_branch", "s_nop", "s_waitcnt", "s_load", "s_endpgm")):
            kinds["SALU"] += 1
    return code, n, branches, nops, to_cmp, to_rfl, kinds


KEEP = None


def main():
    global KEEP
    args = sys.argv[1:]
    if "--keep" in args:
        i = args.index("--keep")
        KEEP = args[i + 1]
        del args[i:i + 2]
        os.makedirs(KEEP, exist_ok=True)
    tmp = KEEP or tempfile.mkdtemp(prefix="isa_audit_")
    try:
        occ = {}
        if args:
            co = extract_code_object(args[0], tmp)
            print("code object of", os.path.basename(args[0]))
        else:
            co, occ = build_code_object(tmp)
            print("device code of the tree, hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize")
        funcs, meta = disassemble(co), metadata(co)
        for label, key in KERNELS:
            sym = [s for s in funcs if key in s and not s.endswith(".kd")]
            if not sym:
                print(label, "not in the code object")
                continue
            code, n, br, nops, c2c, c2r, kinds = audit(funcs[sym[0]])
            md = meta.get(sym[0], {})
            print("%-19s code %6d bytes  %5d instructions  branches %3d  s_nop %3d  v_cndmask 0,1 -> v_cmp_ne %2d  -> v_readfirstlane %2d"
                  % (label, code, n, br, nops, c2c, c2r))
            print("%-19s static mix: %s" % ("", "  ".join("%s %d" % kv for kv in kinds.items())))
            print("%-19s SGPRs %s  VGPRs %s  AGPRs %s  scratch %s  SGPR spills %s  VGPR spills %s  LDS %s  occupancy %s waves/SIMD"
                  % ("", md.get("sgpr_count", "?"), md.get("vgpr_count", "?"), md.get("agpr_count", "?"), md.get("private_segment_fixed_size", "?"),
                     md.get("sgpr_spill_count", "?"), md.get("vgpr_spill_count", "?"), md.get("group_segment_fixed_size", "?"),
                     occ.get(sym[0], "(build to see)")))
    finally:
        if not KEEP:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
