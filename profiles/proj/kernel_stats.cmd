rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o proj -- python tools/proj_timing.py --small --no-cpu
(--small: PCA n = 3 000, F = 2 772; DBSCAN n = 20 000, d = 2; k-means n = 20 000, k = 2, 20 starts; each shape twice)
kernel_stats.csv keeps the 13 frisk_proj kernels (25.1 ms in all; Percentage is of every kernel of the run).  The other 85 rows of
the run were the rocSOLVER / rocBLAS / torch kernels of torch.linalg.eigh and copies: 29 197 launches, 176.9 ms.
