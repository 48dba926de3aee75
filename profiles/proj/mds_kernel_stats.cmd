rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mds -- python tools/proj_timing.py --mds-only --no-cpu --ns 5000
(n = 300 once as a warm-up, then n = 5 000 windows of F = 2 772, d = 2: create + run(Y0, 1, 0) + run(Y0, 21, 0), then the 5-start mds())
mds_kernel_stats.csv keeps the whole run: 3 dissimilarity launches (0.84 ms at n = 300, 6.0 / 5.9 ms at n = 5 000), 65 step passes,
each followed by the one-block sum of its partials (5.8 us).  One step pass at n = 5 000: 140 us, against the 32 us floor of reading 8n^2 bytes of D at 6.3 TB/s.
