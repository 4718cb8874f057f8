#!/usr/bin/env python3
"""isa_equal.py OLD_CSRC NEW_CSRC [--allow NAME ...] -- is the gfx950 device code of two csrc trees the same?

Every device compile of each tree's Makefile (`make -n -B`: the .hip files and the .cpp files built
with -x hip, with the Makefile's own flags) is run with --cuda-device-only -S into a temporary
directory. Per kernel, the assembly text and the resource entries of its metadata are compared
for equality after removing what differs between two compiles of one source or moves when another
function of the file is removed: trailing `;` comments, the function ordinal in local labels and the
__hip_cuid_ symbol. Prints one line per kernel; exits 1 unless every kernel present in both trees is
the same (kernels whose demangled name contains an --allow NAME may differ; for those that do, both
sides' resource entries and spill counts are printed, and for a kernel only the new tree has, its
own). Needs no GPU.
"""
import argparse, collections, concurrent.futures, os, re, shlex, subprocess, sys, tempfile

META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")
SHOWN = (".vgpr_spill_count",)  # printed with META for an allowed kernel that differs, not compared


def device_compiles(csrc):
    out = subprocess.run(["make", "-n", "-B", "-C", csrc], check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        try:
            w = shlex.split(line)
        except ValueError:
            continue
        if "-c" in w and any(a.startswith("--offload-arch") for a in w):
            i = w.index("-c")  # ... -c SRC -o OBJ
            yield w[i + 1], w[:i] + w[i + 4:]


def assembly(csrc, tmp):
    jobs = [(src, cmd + ["--cuda-device-only", "-S", src, "-o", os.path.join(tmp, src + ".s")])
            for src, cmd in device_compiles(csrc)]
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda j: subprocess.run(j[1], cwd=csrc, check=True, stderr=subprocess.DEVNULL), jobs))
    return {src: open(cmd[-1]).read() for src, cmd in jobs}


def normalise(line):
    line = line.split(";")[0].rstrip()
    line = re.sub(r"\.(LBB|Ltmp|Lfunc_end|Lfunc_begin)\d+", r".\1N", line)
    return re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)


def kernels(text):
    """symbol -> (normalised text from its .type line to its .Lfunc_end label, its metadata entries)"""
    body, cur, meta = collections.defaultdict(list), None, {}
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
        if cur and normalise(line):
            body[cur].append(normalise(line))
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
    for item in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):])[1:]:
        sym = re.search(r"\.name:\s+(\S+)", item)
        if sym:
            meta[sym.group(1)] = sorted(l.strip() for l in item.splitlines() if l.strip().split(":")[0] in META + SHOWN)
    return {k: ("\n".join(body[k]), meta.get(k)) for k in body}  # device functions too: no metadata


def compared(kernel):
    text, meta = kernel
    return text, meta and [l for l in meta if l.split(":")[0] in META]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", action="append", default=[], help="kernel name that may differ")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        sides = []
        for i, csrc in enumerate((a.old, a.new)):
            os.mkdir(os.path.join(t, str(i)))
            sides.append(assembly(os.path.abspath(csrc), os.path.join(t, str(i))))
    bad = 0
    for src in sorted(set(sides[0]) | set(sides[1])):
        old, new = (kernels(s.get(src, "")) for s in sides)
        names = sorted(set(old) | set(new))
        demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
        print(f"{src}: {len(old)} kernels in OLD, {len(new)} in NEW")
        for sym, name in zip(names, demangled):
            if sym in old and sym in new:
                state = "same" if compared(old[sym]) == compared(new[sym]) else "DIFFERENT"
                if state != "same":
                    allowed = any(x in name for x in a.allow)
                    bad += not allowed
                    state += " (allowed)" if allowed else ""
            else:
                state = "only in OLD" if sym in old else "only in NEW"
            print(f"  {state:12s} {name.replace('(anonymous namespace)::', '').split('(')[0][:160]}")
            if state.endswith("(allowed)"):
                for side, k in (("OLD", old[sym]), ("NEW", new[sym])):
                    print(f"    {side} " + "  ".join(k[1] or []))
            elif state == "only in NEW" and new[sym][1]:  # (a kernel: device functions have no metadata)
                print("    NEW " + "  ".join(new[sym][1]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
