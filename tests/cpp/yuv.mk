# The program of the 4:2:0 conversion tests (tests/test_yuv_host.py):
#   make -C tests/cpp -f yuv.mk args_yuv
ROOT := $(abspath ../..)
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# The extent and overlap rules of the two conversion entries (csrc/dis_args.h)
# under ASan + UBSan, any finding aborts: compiled and run on the CPU
# (args_yuv_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_yuv_host
args_yuv: args_yuv_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_yuv_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f args_yuv_host
