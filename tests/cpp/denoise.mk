# The program of the temporal-denoising tests (tests/test_denoise_host.py):
#   make -C tests/cpp -f denoise.mk args_denoise
ROOT := $(abspath ../..)
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# The tile grid, the sizes, a weight's bounds and the buffer rules of
# dis_temporal_denoise_u8 (csrc/dis_args.h), under ASan + UBSan, any finding
# aborts: compiled and run (args_denoise_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_denoise_host
args_denoise: args_denoise_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_denoise_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f args_denoise_host
