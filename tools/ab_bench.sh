# A/B timing of two builds ON THE SAME GPU BOX (boxes differ by up to 5 %): put the two libraries into ab/libA.so and ab/libB.so
# (ab/ is git-ignored), then: bash tools/ab_bench.sh [bench args].  Three alternating rounds; the libraries are chosen with
# SURFEL_RASTER_LIB, which the loader takes as it is (the in-tree library must carry the tree's source digest, a parent build does not).
for r in 1 2 3; do for v in ${AB_VARIANTS:-A B}; do
  SURFEL_RASTER_LIB=$PWD/ab/lib$v.so timeout 170 python bench.py --full --no-cpu-baseline --no-train-step "$@" 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['value'], d['ms_per_step'], {k: (None if x is None else round(x, 4)) for k, x in d['stage_ms'].items()})"
done; done
