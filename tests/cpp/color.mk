# The programs of the colour frame input tests (tests/test_color_host.py):
#   make -C tests/cpp -f color.mk [png_rgb_tool | luma_check | args_color]
ROOT := $(abspath ../..)
CLI := $(ROOT)/optical-flow-using-dense-inverse-search_amd/cli
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc
all: png_rgb_tool luma_check

# the colour side of the codec (png::read_rgb / write_rgb) and the host luma
# over all 2^24 colours against a table
png_rgb_tool: png_rgb_tool.cpp $(CLI)/png.hpp
	g++ -std=c++17 -O2 -Wall -I$(CLI) $< -o $@ -lz
luma_check: luma_check.cpp $(CLI)/png.hpp
	g++ -std=c++17 -O2 -Wall -I$(CLI) $< -o $@ -lz

# The frame-batch rule with a pixel size (csrc/dis_args.h) under ASan + UBSan,
# any finding aborts: compiled and run (args_color_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_color_host
args_color: args_color_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_color_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f png_rgb_tool luma_check args_color_host
