"""lorikeet_amd -- MI355X-native PairHMM read x haplotype likelihood engine (drop-in for the
PairHMM path of rhysnewell/Lorikeet).  See DESIGN.md / INTEGRATION.md.

Only what the path needs lives here: `csrc/` (gfx950 kernels + the C ABI of include/phmm.h) and
the host-side mirror of the reference interface.  Importing the package does not need a GPU;
creating an engine does (there is no CPU fallback).
"""
from .activity import activity_profile  # noqa: F401
from .finalize import finalize_reads  # noqa: F401
from .phase import phase_calls  # noqa: F401
from .assembly import apply_recovery, assembly_graph, assembly_kmers, best_paths, prune_graph, recover_dangling_ends, sequence_graph  # noqa: F401
from .trim import trim_regions  # noqa: F401
from .assembly_regions import assembly_regions  # noqa: F401
from .batch import Read, RegionBatch  # noqa: F401
from .engine import HipPairHMMEngine, PhmmError  # noqa: F401
from .events import discover_events  # noqa: F401
from .genotype import annotate_events, allele_frequency, assign_genotypes, genotype_likelihoods  # noqa: F401
