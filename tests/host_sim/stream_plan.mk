# tests/host_sim/stream_plan.mk: the single stream's launch plan (nlzm_amd/csrc/nlzm_stream_plan.h) in a program of its own, under
# AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_stream_plan.py).
DEPS = stream_plan_sim.cpp ../../nlzm_amd/csrc/nlzm_stream_plan.h
all: stream_plan_sim_san
stream_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ stream_plan_sim.cpp
clean:
	rm -f stream_plan_sim_san
