// A stand-alone program around vrhip_render's option parser and refusals (volumerenderercl_amd/csrc/host/vrhip_cli.cpp),
// for the host sanitizers: tests/test_cli_args.py compiles that file together with this one with
// -fsanitize=address,undefined and runs the result once per argument vector (a refusal ends the process, as in the
// CLI).  No device, no library: the arguments of this program are the arguments of vrhip_render.
#include <vrhip_cli.h>

#include <cstdio>

int main(int argc, char **argv)
{
    const Options o = parse_args(argc, argv);
    validate(o);
    validate_easing(o);
    validate_source_and_output(o);
    std::printf("accepted: size %zu %zu frames %d filters %zu\n", o.view.W, o.view.H, o.batch.frames, o.filters.size());
    return 0;
}
