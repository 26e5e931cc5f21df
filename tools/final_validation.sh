# round-end validation on the GPU box: tests, smoke, the bench workloads (--full: roofline, variants, CPU baseline), rocprofv3 kernel stats, PMC passes
#   [OUT=<dir>] bash tools/final_validation.sh <tag> [quick]      quick: skip the variant benches and the PMC passes; all outputs -> OUT (default validation_out/)
export TMPDIR=/tmp
R=$PWD
OUT=${OUT:-$R/validation_out}
TAG=${1:-r06}
QUICK=${2:-}
mkdir -p $OUT
rm -f $R/gpurun_out/qwen_full_drift.txt $R/gpurun_out/qwen_outliers_drift.txt $R/gpurun_out/sft_full_drift.txt $R/gpurun_out/sft_navdp_drift.txt $R/gpurun_out/s1_b64_distribution.txt
timeout 2400 python -m pytest tests -q -m gpu > $OUT/${TAG}_pytest_gpu.log 2>&1
for f in qwen_full_drift qwen_outliers_drift sft_full_drift sft_navdp_drift s1_b64_distribution; do cp $R/gpurun_out/$f.txt $R/gpurun_out/${TAG}_$f.txt 2>/dev/null; done
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
timeout 900 python bench.py --full > $OUT/${TAG}_bench_n1_dual_b64.json 2> $OUT/${TAG}_bench.err
if [ -z "$QUICK" ]; then
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --cadence reference > $OUT/${TAG}_bench_n1_dual_b64_reference.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload s2_only > $OUT/${TAG}_bench_s2_only_b7.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --num-history 8 --lookdown --steps 10 > $OUT/${TAG}_bench_n1_dual_b64_h8_lookdown.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --prefix-kv --steps 20 > $OUT/${TAG}_bench_n1_dual_b64_prefixkv.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload navdp_s1 > $OUT/${TAG}_bench_navdp_s1_b64.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload unet1d_s1 --no-cpu-baseline > $OUT/${TAG}_bench_unet1d_s1_b64.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload sft --steps 30 --warmup 3 --no-cpu-baseline > $OUT/${TAG}_bench_sft.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload sft --steps 30 --warmup 3 --no-cpu-baseline --no-prefetch > $OUT/${TAG}_bench_sft_noprefetch.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload sft --steps 30 --warmup 3 --no-cpu-baseline --no-priority > $OUT/${TAG}_bench_sft_nopriority.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --workload sft --steps 30 --warmup 3 --no-cpu-baseline --no-graph-prefix > $OUT/${TAG}_bench_sft_eagerprefix.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --dit-ffn 1024 > $OUT/${TAG}_bench_n1_dual_b64_ffn1024.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --no-frag-weights > $OUT/${TAG}_bench_n1_dual_b64_no_frag_weights.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --no-row-chain > $OUT/${TAG}_bench_n1_dual_b64_no_row_chain.json 2>> $OUT/${TAG}_bench.err
timeout 600 python bench.py --full --no-cpu-baseline --no-variants --no-fuse-decode-rope > $OUT/${TAG}_bench_n1_dual_b64_no_fuse_decode_rope.json 2>> $OUT/${TAG}_bench.err
timeout 300 python bench.py --full --workload host_stub --gpus 8 --steps 20 > $OUT/${TAG}_bench_host_stub_8ranks.json 2>> $OUT/${TAG}_bench.err
fi
timeout 300 python tools/step_breakdown.py > $OUT/${TAG}_step_breakdown.log 2>&1
cd /tmp
timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/kt -o kt -- python $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-variants > $OUT/kt.log 2>&1
python $R/tools/rocprof_summary.py $(ls $OUT/kt/*.db | head -1) 45 > $OUT/${TAG}_n1_dual_b64_kernel_stats.txt 2>&1
rm -rf $OUT/kt
for w in s1 s2; do
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/kt_$w -o kt -- python $R/tools/profile_phases.py $w 3 > $OUT/kt_$w.log 2>&1
python $R/tools/rocprof_summary.py $(ls $OUT/kt_$w/*.db | head -1) 40 > $OUT/${TAG}_${w}_3calls_kernel_stats.txt 2>&1
rm -rf $OUT/kt_$w
done
if [ -z "$QUICK" ]; then
# PMC passes (counters alone, --kernel-trace only): HBM-side traffic and SQ counters of one eager System-2 call (the timed step's launches)
timeout 420 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pf -o f -- python $R/tools/profile_phases.py s2 1 > $OUT/pf.log 2>&1
timeout 420 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pw -o w -- python $R/tools/profile_phases.py s2 1 > $OUT/pw.log 2>&1
python $R/tools/pmc_summary.py $OUT/pf/f_results.db $OUT/pw/w_results.db 14 > $OUT/${TAG}_pmc_hbm_traffic_s2_call.txt 2>&1
rm -rf $OUT/pf $OUT/pw
for w in s1 s2; do
timeout 420 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS --kernel-trace -d $OUT/ps -o s -- python $R/tools/profile_phases.py $w 1 > $OUT/ps.log 2>&1
{ python $R/tools/pmc_sq_summary.py $OUT/ps/s_results.db 14; python $R/tools/pmc_table.py $OUT/ps/s_results.db 14; } > $OUT/${TAG}_pmc_sq_${w}_call.txt 2>&1
rm -rf $OUT/ps
done
fi
# torch-free native probes over the C-ABI (seconds each). Rebuilt here against the header of THIS tree: a probe compiled before a struct of
# include/internnav_amd.h changed hands the library a mis-laid argument block (a GPU memory fault in round 6)
cd $R
bash tools/native/build.sh > $OUT/${TAG}_native_build.log 2>&1
if [ -x tools/native/chain_sweep ]; then
  timeout 90 tools/native/gemm_sweep internnav_amd/libinternnav_amd.so tools/native/specs_r04_rowpanel.txt > $OUT/${TAG}_native_rowpanel.log 2>&1
  timeout 90 tools/native/gemm_sweep internnav_amd/libinternnav_amd.so tools/native/specs_r04_w4.txt > $OUT/${TAG}_native_w4.log 2>&1
  timeout 90 tools/native/chain_sweep internnav_amd/libinternnav_amd.so tools/native/specs_r04_w4_chain.txt spec > $OUT/${TAG}_native_w4_chain.log 2>&1
  timeout 60 tools/native/chain_sweep internnav_amd/libinternnav_amd.so all part > $OUT/${TAG}_native_chain_partitions.log 2>&1
  timeout 60 tools/native/chain_sweep internnav_amd/libinternnav_amd.so tools/native/specs_r04_phase_mix.txt spec > $OUT/${TAG}_native_phase_mix.log 2>&1
  timeout 30 tools/native/skinny_sweep internnav_amd/libinternnav_amd.so 6 > $OUT/${TAG}_native_skinny.log 2>&1
  timeout 20 tools/native/attn_probe internnav_amd/libinternnav_amd.so > $OUT/${TAG}_native_attn.log 2>&1
  timeout 120 tools/native/gemm_sweep internnav_amd/libinternnav_amd.so tools/native/specs_r05_w4p.txt > $OUT/${TAG}_native_w4p.log 2>&1
  timeout 60 tools/native/dit_attn_probe internnav_amd/libinternnav_amd.so > $OUT/${TAG}_native_dit_attn.log 2>&1
  timeout 60 tools/native/rowchain_probe internnav_amd/libinternnav_amd.so 1536 > $OUT/${TAG}_native_rowchain.log 2>&1
  timeout 60 tools/native/rowchain_probe internnav_amd/libinternnav_amd.so 1024 > $OUT/${TAG}_native_rowchain_ffn1024.log 2>&1
  timeout 60 tools/native/issue_cost_probe > $OUT/${TAG}_native_issue_cost.log 2>&1
fi
tail -3 $OUT/${TAG}_pytest_gpu.log
tail -2 $OUT/${TAG}_smoke.log
head -c 400 $OUT/${TAG}_bench_n1_dual_b64.json; echo
head -12 $OUT/${TAG}_step_breakdown.log
tail -6 $OUT/${TAG}_bench.err
