"""Binning walks (bin_kernel<false/true>): threads per workgroup.  (The three *_nopf entries, which also switched off the request of
the next step's loads a step ahead -- S3G_BIN_PREFETCH 0, measured slower in round 4 -- last applied at commit 72424ac: the
prefetching walk is the only one since; their numbers stay in profiles/.)"""
T = "#define S3G_BIN_THREADS 512"
VARIANTS = {
    "bin_256": ("raster_bin.hip", [(T, "#define S3G_BIN_THREADS 256")]),
    "bin_1024": ("raster_bin.hip", [(T, "#define S3G_BIN_THREADS 1024")]),
}
