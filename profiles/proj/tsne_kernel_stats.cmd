rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o tsne -- python tools/proj_timing.py --small --no-cpu --tsne-only
(--small --tsne-only: PY-TSNE at n = 1 000 windows of F = 2 772 -> 50 columns, d = 2, perplexity 20, 1000 iterations, once)
tsne_kernel_stats.csv keeps the 15 frisk_tsne_impl / frisk_proj kernels (39.1 ms in all; Percentage is of every kernel of the run).
The other 85 rows of the run were the rocSOLVER / rocBLAS / torch kernels of torch.linalg.eigh and copies: 14 172 launches, 85.7 ms.
At n = 1 000 an iteration is five launches of 4.6 - 16.8 us each (38 us in all): launch-bound; see DESIGN.md section 9 for n >= 5 000.
