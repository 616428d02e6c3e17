#!/bin/bash
# tools/ktext_diff.sh TREE_A TREE_B — device code of two trees of this repository, compared function by function, without a GPU.
# Every unit of `build.py --print-units` of each tree is compiled for gfx950 with the library's flags plus `--cuda-device-only -S`
# (at most 8 compilers at a time), the `__hip_cuid_` lines (a hash of the source) are dropped, and the assembly is split where a function
# begins: a function's part holds its instructions, its `.amdhsa_*` block and the resource lines behind it. Prints `identical N of M`
# and the demangled name of every function whose part differs or that only one tree has; exit status 1 if any does. Text is compared
# as text; nothing is looked for in it.
# KTEXT_WORK=dir keeps the assembly in dir/<source id of the tree>/ and compiles a tree with the same sources only once; the compilers'
# messages stand beside it in *.log. KTEXT_FLAGS adds flags (the directory's name then ends in their checksum):
# -Rpass-analysis=kernel-resource-usage leaves in the logs what tools/kres2.sh reads.
set -euo pipefail
[ $# -eq 2 ] || { echo "usage: $0 TREE_A TREE_B" >&2; exit 2; }
PKG=highperformancecomputing-latticeboltzmannmethod_amd
WORK=${KTEXT_WORK:-$(mktemp -d)}
[ -n "${KTEXT_WORK:-}" ] || trap 'rm -rf "$WORK"' EXIT
HIPCC=$(command -v hipcc || echo "${ROCM_PATH:-/opt/rocm}/bin/hipcc")

assemble() {      # $1: tree; prints the directory that holds one .s per unit
    local tree id out src obj flags
    tree=$(cd "$1" && pwd)
    id=$(cd "$tree/$PKG" && python3 -c "import build; print(build.source_id())")
    out="$WORK/$id${KTEXT_FLAGS:+-$(printf %s "$KTEXT_FLAGS" | cksum | cut -d" " -f1)}"
    if [ ! -e "$out/.done" ]; then
        mkdir -p "$out"
        while IFS=$'\t' read -r src obj flags; do
            while [ "$(jobs -rp | wc -l)" -ge 8 ]; do wait -n; done
            # ($flags unquoted: split into words, its quotes kept as build.py passes them)
            "$HIPCC" --offload-arch=gfx950 -O3 -std=c++20 -ffp-contract=off -fPIC -pthread $flags ${KTEXT_FLAGS:-} --cuda-device-only -S \
                -o "$out/${obj%.o}.s" "$tree/$PKG/csrc/$src" 2> "$out/${obj%.o}.log" || echo "$obj" >> "$out/.failed" &
        done < <(python3 "$tree/$PKG/build.py" --print-units)
        wait
        [ ! -e "$out/.failed" ] || { echo "$tree: did not compile: $(tr '\n' ' ' < "$out/.failed")(logs in $out)" >&2; rm "$out/.failed"; exit 2; }
        touch "$out/.done"
    fi
    echo "$out"
}

A=$(assemble "$1")
B=$(assemble "$2")
python3 - "$A" "$B" <<'PY'
import glob, os, re, subprocess, sys

def parts(d):
    """{(unit, function): text} of every unit's assembly in d; what precedes a unit's first function and its metadata are parts too."""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit, name, cur = os.path.basename(path)[:-2], "(head)", []
        for line in open(path):
            if "__hip_cuid_" in line or line.startswith("\t.section\t.text"):
                continue
            m = re.search(r"; -- Begin function (\S+)", line)
            if m or line.startswith("\t.amdgpu_metadata"):
                out[(unit, name)] = "".join(cur)
                name, cur = (m.group(1) if m else "(metadata)"), []
            cur.append(line)
        out[(unit, name)] = "".join(cur)
    return out

a, b = parts(sys.argv[1]), parts(sys.argv[2])
keys = sorted(set(a) | set(b))
bad = [k for k in keys if a.get(k) != b.get(k)]
print("identical %d of %d (%d units)" % (len(keys) - len(bad), len(keys), len({u for u, _ in keys})))
if bad:
    dem = subprocess.run(["c++filt"], input="\n".join(n for _, n in bad), capture_output=True, text=True).stdout.split("\n")
    for (unit, _), n in zip(bad, dem):
        why = "differs" if (unit, _) in a and (unit, _) in b else ("only in the first tree" if (unit, _) in a else "only in the second tree")
        print("%s: %s: %s" % (unit, n, why))
sys.exit(1 if bad else 0)
PY
