// tree_units.hip — the DEEP division, FRI fold, Merkle tree, FRI forest, path
// and shard-layout units as one translation unit, so that their kernels share
// one code object, as they did in merkle.hip. Each unit also compiles on its
// own to the same kernels, but as six code objects the three-proofs-in-flight
// rate fell into a mode about 1 % lower in 19 of 31 runs, against 2 of 23 for
// the parent and 2 of 14 for this form (profiles/merkle_split/bench_ab.txt);
// a single proof and every kernel's own time did not differ.
#include "deep_div.hip"
#include "fri_fold.hip"
#include "merkle_tree.hip"
#include "fri_forest.hip"
#include "fri_paths.hip"
#include "shard_layout.hip"
