"""The operation-sequence fuzz (tests/sequence_fuzz_common.py) on the HIP engine: random sequences of ingests, finalizes, plane
and flag pointers, flag unions and checkpoints on one pipeline, in core and out of core, held bit for bit to the model that
tests/test_sequence_fuzz_host.py has pinned on the host engine.  What it is for is the layer that decides which buffer a kernel
reads and whether it runs at all (the plane-state block of host/src/device_pipeline.cpp, LeavingBand{raw, out}): on the seeds
the generator marks, the first ingest must have stored its bands (and left planes in them), so the sequence behind it walks the
stale-band and plane-restore paths.  Every finalize plan carries a drawn PipelineConfig.terrain list, so the last rows of that
table -- terrain bands of every kind of source, in core and out of core -- are held to the NumPy model of the contract too; the
list does not switch the offer off, and the assertions on the marked seeds stand.  The 52 default seeds in the suite;
PCR_SEQ_FUZZ_SEEDS=a:b soaks a range (or a,b,c: those seeds).  A failure names its seed, the index of the op and the band.

The line cases (LINE_SEEDS; any seed from LINE_SEED_BASE on, so PCR_SEQ_FUZZ_SEEDS=2000:2400 soaks them) add Line groups and
a Point WeightedAverage: exact sums again (a visit has weight 1), so the Line tile kernels' fixed-point window, list and rescan,
the listed and the direct path and the plane-state rules for glyph groups are held to the oracle's footprint bit for bit.
Gaussian groups are not drawn (expf weights: no exact model).  The generator's _line_pass keeps every Line sum exact.
last_scatter() reports the last scatter of an ingest, which in a line case is the last Line group's: where the binned path is
forced, and on the hot and late-large clouds, check_sequence asserts that it went through the tile kernels.

The accumulator cases (ACC_SEEDS; any seed from ACC_SEED_BASE on, so PCR_SEQ_FUZZ_SEEDS=10400:12400 soaks them) run one in-core
pipeline with per-reduction filters, surface channels, histograms, extremes, cell stats, tree bands and zonal tables at once:
the point mask across the scatters of one ingest, the scatter path per cloud, the band order and fill rules over every band
kind, and what trees(i) / zonal(i) answer after pointers were handed out, planes written, flags merged, a checkpoint call refused
or nothing happened -- every state, band and table bit for bit against the features' own integer models.

The polygon cases (POLY_SEEDS; any seed from POLY_SEED_BASE on, so PCR_SEQ_FUZZ_SEEDS=20000:20400 soaks them) put polygon
channels, point zonal tables, polygon-burnt zone grids and polygonize on top of an accumulator case: the per-ingest staging
buffer of a polygon channel read by the filter classes, every scatter, every accumulator and the point zonal fold on one
stream; set_polygons between ingests, also right behind an ingest_async nobody waited for and before a larger cloud that grows
the staging buffer; the early return for an emptied cloud, which must leave the tables as they were; points outside the grid
that count in the tables and in no scatter; chunked ingest_file; outlines under zonal's freshness rule, with Host and Device
results; and the round trip polygonize -> set_zones -> zonal against the by-band table.  The clouds come from host, page-locked and device
memory and from files, as the seed draws it for every family."""
import pytest

import pcr
import sequence_fuzz_common as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", S.seeds_from_env())
def test_sequence_on_the_hip_engine_equals_the_model(seed, tmp_path):
    S.check_sequence(seed, pcr.ExecutionMode.GPU, "hip", tmp_path)
