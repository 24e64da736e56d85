D=${1:?usage: diag_uconv_run.sh <output folder>}/d1
mkdir -p $D
for v in "" _uconvd1 _uconvd2 _uconvd3; do
  LDM_AMD_LIB=$PWD/music-style-transfer-ldm_amd/lib/libldm_amd$v.so timeout -k 10 120 python -u tools/step_times.py --no-loop --variant uconv > $D/times$v.txt 2>&1 || exit 1
done
LDM_AMD_LIB=$PWD/music-style-transfer-ldm_amd/lib/libldm_amd_uconvd4.so timeout -k 10 120 python -u tools/step_times.py --no-loop --variant uconv --stamps > $D/stamps.txt 2>&1 || exit 1
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $D/bench.json 2> $D/bench.err || exit 1
tail -n 12 $D/*.txt
python3 -c "import json;d=json.load(open('$D/bench.json'));print(d['value'],d['us_per_denoise_iteration']);[print(k,v['us'],v['kernel']) for k,v in d['kernels'].items()]"
