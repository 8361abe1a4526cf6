"""What a run launched, from a rocprofv3 kernel trace (`rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- <program>`):

    python tools/launch_sequence.py DIR/.../t_kernel_trace.csv [--filter REGEX]

Per hardware queue, in dispatch order: the kernel's short name with its template arguments, the grid size and the workgroup size.  Only the
path tracer's kernels are kept (the filter of tools/kernel_isa_stats.sh in profiles/r25/kernel_isa_identity.txt).  The queues are printed sorted
by their content and numbered in that order, so that which lane's stream got which queue, and which lane started first, do not matter: two
builds launched the same things on the same number of queues when `diff` of their listings is empty."""
import argparse
import csv
import re

FILTER = r"k_trace|k_shade|k_raygen|k_resolve\b|k_direct|k_first_hit|k_accumulate|trhip_spec"


def short_name(kernel_name):
    """'void tr::(anonymous namespace)::k_shade<false, true, tr::(anonymous namespace)::SpecCli>(tr::SceneView, ...) [clone .kd]' ->
    'k_shade<false, true, SpecCli>'"""
    m = re.search(r"(k_[A-Za-z_0-9]+|trhip_spec[A-Za-z_0-9]*)", kernel_name)
    if not m:
        return None
    name, rest = m.group(1), kernel_name[m.end():]
    if rest.startswith("<"):      # the template arguments: up to the matching '>'
        depth = 0
        for i, ch in enumerate(rest):
            depth += ch == "<"
            depth -= ch == ">"
            if depth == 0:
                name += re.sub(r"\b(?:tr::)?(?:\(anonymous namespace\)::)?", "", rest[:i + 1])
                break
    return name


def size_of(row, what):
    """Grid_Size / Workgroup_Size of older rocprofv3 releases, or the _X, _Y, _Z columns of newer ones."""
    if row.get(what) not in (None, ""):
        return row[what]
    dims = [row.get(f"{what}_{d}") for d in "XYZ"]
    if dims[0] in (None, ""):
        raise SystemExit(f"no {what} column in the trace: {sorted(row)}")
    dims = [int(d) for d in dims if d not in (None, "")]
    return str(dims[0]) if all(d == 1 for d in dims[1:]) else "x".join(str(d) for d in dims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--filter", default=FILTER)
    args = ap.parse_args()
    queues = {}
    for n, row in enumerate(csv.DictReader(open(args.trace))):
        if not re.search(args.filter, row["Kernel_Name"]):
            continue
        name = short_name(row["Kernel_Name"])
        if name is None:
            continue
        order = (int(row["Dispatch_Id"]) if row.get("Dispatch_Id") else int(row["Start_Timestamp"]), n)
        queue = (row.get("Agent_Id", ""), row.get("Queue_Id", ""))
        queues.setdefault(queue, []).append((order, f"{name}  grid {size_of(row, 'Grid_Size')}  workgroup {size_of(row, 'Workgroup_Size')}"))
    listings = sorted([line for _, line in sorted(q)] for q in queues.values())
    for i, lines in enumerate(listings):
        print(f"== queue {i}: {len(lines)} launches")
        for line in lines:
            print(line)


if __name__ == "__main__":
    main()
