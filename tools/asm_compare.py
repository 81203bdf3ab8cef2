"""Are two builds of the device code the same program?  Compares two device assemblies (hipcc --cuda-device-only -S, the command
of tests/test_build_isa.py) kernel by kernel: the instruction stream with its labels and the kernel descriptor (.amdhsa_*), without
what depends on source positions (comments, .loc / .file / .cfi directives, debug sections).  No GPU needed.
  python3 tools/asm_compare.py OLD.s NEW.s        exit status 1 if a kernel differs or exists on one side only"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        text = line.split(";")[0].strip()
        if text.startswith(".Lfunc_end"):   # (the kernel descriptor, .amdhsa_kernel ... .end_amdhsa_kernel, lies before it: part of the body)
            out[name], name = body, None
        elif text and not re.match(r"\.(loc|file|cfi_\w+)\b", text):
            # (a block label carries the number of its function in the file, .LBB<function>_<block>: kernels added or removed in front of
            # this one renumber it and change nothing else)
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = [k for k in old if k in new and old[k] != new[k]]
    only = sorted(set(old) ^ set(new))
    same = sum(1 for k in old if k in new and old[k] == new[k])
    for k in differ:
        at = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
        print(f"DIFFERS {k}: {len(old[k])} / {len(new[k])} lines, first at {at}")
    for k in only:
        print(f"ON ONE SIDE ONLY {k}")
    print(f"{len(old)} kernels with their descriptors ({sum(1 for k in old if 'photon_kernel' in k)} of photon_kernel): "
          f"{same} identical, {len(differ)} differ, {len(only)} on one side only")
    sys.exit(1 if differ or only else 0)


main()
