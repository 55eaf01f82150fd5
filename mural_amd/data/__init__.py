from .genome import PackedGenome, SymbolWindows, pack_sequence, label_sites, label_sites_host, new_label_stats, site_selection, class_mask, split_rows, scatter_rows  # noqa: F401
from .ingest import read_fasta, read_bed, bed_order, predict_bed, scan_fasta, pack_fasta_record, poisson_calibrate, write_predictions, packed_segments, train_batches_from_files, read_mutations  # noqa: F401
from .loader import EpochLoader, EpochView, ViewRows  # noqa: F401
