"""One rank of the sharded composed driver (tests/test_gpu_composed_sharded.py): RANK / WORLD_SIZE / MASTER_* from the
environment, Gloo for the two small exchanges (every rank of the test shares the box's one GPU, which RCCL does not take),
the composed fixture `sys.argv[1]` of tests/golden/composed_vectors.npz, output `sys.argv[2]`, working directory
`sys.argv[3]`; an optional `sys.argv[4]` names a many-contig fixture file (tests/golden/composed_many_contigs.npz) to run
instead."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def many_contig_inputs(path):
    """(chromosomes, args, {chromosome: (locus starts, K x n matrix)}, combined BED text) of a many-contig fixture
    (tests/golden/make_golden_composed.py, part 3): the tracks are stored in hundredths, the loci as start and length."""
    gold = np.load(path)
    chroms = [str(c) for c in gold["chroms"]]
    ends = np.cumsum(gold["lengths"])
    inputs = {}
    for c, start, n, end in zip(chroms, gold["starts"].tolist(), gold["lengths"].tolist(), ends.tolist()):
        inputs[c] = (start + np.arange(n, dtype=np.int64) * 50, gold["tracks_hundredths"][:, end - n:end] / 100.0)
    return chroms, json.loads(str(gold["args"][0])), inputs, str(gold["combined_bed"][0])


def main():
    import torch.distributed as dist

    from rocco_amd import rocco as impl

    fixture, output, workdir = sys.argv[1], sys.argv[2], sys.argv[3]
    if len(sys.argv) > 4:
        chroms, args, inputs, _want = many_contig_inputs(sys.argv[4])
    else:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "composed_vectors.npz"))
        chroms = [str(c) for c in gold[f"{fixture}_chroms"]]
        args = json.loads(str(gold[f"{fixture}_args"][0]))
        inputs = {c: (gold[f"{fixture}_{c}_intervals"], gold[f"{fixture}_{c}_matrix"]) for c in chroms}
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    os.makedirs(os.path.join(workdir, f"rank{rank}"), exist_ok=True)
    os.chdir(os.path.join(workdir, f"rank{rank}"))  # per-chromosome and summit files go to the working directory
    args["output"] = output
    args["narrowPeak"] = fixture.startswith("counts")
    final = impl.run_chromosomes(chroms + ["chrMissing"], inputs, args, run_id="31")
    left = sorted(os.listdir("."))
    print(json.dumps({"rank": rank, "final": final, "left_in_workdir": left}), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
