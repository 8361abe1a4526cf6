#!/bin/bash
# usage: kernel_isa_stats.sh <host object or shared library with a .hip_fatbin section | gfx950 code object> [name filter]
# Prints, per gfx950 kernel: instructions, VGPRs, SGPRs, scratch bytes, LDS bytes (from the code object's metadata and disassembly) and a
# short hash of the kernel's instruction text - mnemonics and operands only, without address, encoding and comment, so that it does not
# depend on where the kernel lies in the file.  Two builds have the same code for a kernel when their lines are equal: `diff` of two
# outputs is the identity check.  A library linked from several objects holds one bundle per object; all of them are listed.
set -e
obj="$1"; filt="${2:-.}"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
if [ "$(head -c 4 "$obj" | tail -c 3)" = "ELF" ] && /opt/rocm/lib/llvm/bin/llvm-readelf -h "$obj" | grep -q "AMDGPU"; then
    cp "$obj" "$tmp/code0.co"
else
    objcopy -O binary --only-section=.hip_fatbin "$obj" "$tmp/fatbin"
    # one bundle per linked object, each starting with the bundler's magic string
    python3 - "$tmp" <<'PY'
import re, sys
tmp = sys.argv[1]
d = open(tmp + "/fatbin", "rb").read()
starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", d)]
for i, s in enumerate(starts):
    open("%s/bundle%d" % (tmp, i), "wb").write(d[s:starts[i + 1] if i + 1 < len(starts) else len(d)])
PY
    i=0
    while [ -f "$tmp/bundle$i" ]; do
        /opt/rocm/lib/llvm/bin/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$tmp/bundle$i" --output="$tmp/code$i.co" --unbundle
        i=$((i + 1))
    done
fi
for co in "$tmp"/code*.co; do
    [ -s "$co" ] || continue
    /opt/rocm/lib/llvm/bin/llvm-objdump -d "$co" > "$co.dis"
    /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$co" > "$co.notes"
done
python3 - "$tmp" "$filt" <<'PY'
import glob, hashlib, re, sys, subprocess
tmp, filt = sys.argv[1], sys.argv[2]
for dis in sorted(glob.glob(tmp + "/code*.co.dis"), key=lambda p: int(re.search(r"code(\d+)", p).group(1))):
    counts, text, cur = {}, {}, None
    for line in open(dis):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = m.group(1); counts[cur] = 0; text[cur] = hashlib.sha256(); continue
        if cur and re.match(r"^\s+[a-z_0-9]+ ", line) and "//" in line:
            counts[cur] += 1
            text[cur].update((" ".join(line.split("//")[0].split()) + "\n").encode())
    # the metadata: one map per kernel, `  - .key: value` opening it and `    .key: value` continuing it (deeper lines belong to lists inside)
    kernels, k = [], None
    for line in open(dis[:-4] + ".notes"):
        m = re.match(r"^  - \.(\w+):\s*(\S*)", line)
        if m:
            k = {m.group(1): m.group(2)}; kernels.append(k); continue
        m = re.match(r"^    \.(\w+):\s+(\S+)", line)
        if m and k is not None:
            k[m.group(1)] = m.group(2)
    for k in kernels:
        name = k.get("name")
        if not name or "vgpr_count" not in k: continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if not re.search(filt, dem): continue
        g = lambda key: k.get(key, "?")
        h = text[name].hexdigest()[:12] if name in text else "?"
        print(f"{counts.get(name, '?'):>7} instr  vgpr {g('vgpr_count'):>3}  sgpr {g('sgpr_count'):>3}  scratch {g('private_segment_fixed_size'):>4}  lds {g('group_segment_fixed_size'):>6}  {h}  {dem[:110]}")
PY
