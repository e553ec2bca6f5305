// repitch.hip -- Audio::repitch (Audio/AudioTemporal.cpp:236-299): variable-rate resampling through WDL_Resampler's 64-tap windowed
// sinc (WDL/resample.cpp), the rate changing every `granularity` input frames.  DESIGN.md section 4.13.
//
// The reference feeds one resampler block after block on one thread.  Its state between blocks is two numbers (the fractional read
// position and how many samples stay buffered), which a host loop reproduces exactly in fp64 (repitch_plan: O( output frames )
// additions); after that every output sample is an independent 64-tap sum (two of them, interpolated, unless the rates are "ideal")
// over a window of one continuous stream: 31 zeros, the input, zeros.  The resampler itself -- the choice of table, the table, the tap
// sums, the stream -- is wdl_sinc.h's, shared with spatial.hip and wavetable.hip; the plan, the runs and the kernels around them are this file's.
//   k_wdl_window<64>   the Blackman-Harris factor of every table entry, per oversize in use, in fp64 (once per call)
//   k_repitch_sinc     one workgroup per run of consecutive blocks that share a coefficient table: builds the table in LDS, stages the
//                      run's input window in LDS when it fits, one output sample per thread per channel
//   k_repitch_point    the Uninterpolated quality: in[ int( srcpos ) ]
// Every sum runs in a fixed order and nothing is atomic, so two runs agree bit for bit.
#include "wdl_sinc.h"

namespace flanhip {

namespace {

constexpr int RP_TAPS = 64;                    // SetMode( true, 0, true, 64 ): m_sincsize
using Rp = WdlSinc<RP_TAPS>;
constexpr int RP_THREADS = WDL_THREADS;
constexpr int RP_WINDOW_FLOATS = 6144;         // the staged input window of a run (24 KiB); a longer one is read from global memory
constexpr int RP_RUN_OUTPUTS = 2048;           // output frames per run at most (8 per thread)
constexpr int64_t RP_MAX_FRAMES = int64_t( 1 ) << 40;
constexpr int64_t RP_MAX_WORK = int64_t( 1 ) << 33;     // blocks x granularity the host loop accepts (its additions)
constexpr int64_t RP_MAX_BLOCKS = int64_t( 1 ) << 22;   // blocks a call may have: 56 bytes of record each on the host and in the workspace (224 MiB)

struct RpBlock                                 // one call of ResamplePrepare / ResampleOut
	{
	int64_t offset;                            // stream index of the buffer's first sample
	double fracpos;                            // srcpos of the block's first output sample, relative to offset
	double ratio;
	double filtpos;
	int64_t first_out;
	int32_t oversize, ideal;
	int32_t wanted, pad;
	};

struct RpRun                                   // consecutive blocks that share ( filtpos, oversize ): one workgroup per ( run, channel group )
	{
	int64_t first_block;
	int32_t num_blocks, oversize;
	double filtpos;
	int64_t win_start;                         // stream index of the first staged sample
	int32_t win_len, ideal;                    // staged samples (0: read global memory)
	};
static_assert( sizeof( RpBlock ) == 56 && sizeof( RpRun ) == 40, "the device reads these records as the host lays them out" );

struct RpPlan
	{
	std::vector<RpBlock> blocks;
	int64_t out_frames = 0;
	};

// FunctionSample<float>::accumulate() of a vector (FunctionSample.h:136-148: std::accumulate from float()), times g in fp32, ceil (:252)
int64_t rp_out_frames( const float * inv, int64_t count, int64_t g )
	{
	float sum = 0.0f;
	for( int64_t i = 0; i < count; ++i ) sum = sum + inv[i];
	const float frames = std::ceil( sum * float( g ) );
	if( !( frames > 0.0f ) ) return 0;
	return frames >= 9.0e18f ? INT64_MAX : int64_t( frames );
	}

// The block loop of :267-296 with the state of ResamplePrepare (:1218-1265) and ResampleOut (:1313, :1558-1566), in fp64 with the
// reference's own chain of srcpos += ratio.  keep: store the records (else count only).  FLANHIP_OK, or why the loop cannot run.
int rp_plan( int64_t n, float sr, const float * inv, int64_t count, int64_t g, int quality, bool keep, RpPlan * out, int64_t * num_blocks )
	{
	const int fsize = quality == FLANHIP_REPITCH_SINC ? RP_TAPS : 0;
	const int64_t prelude = fsize ? Rp::PRELUDE : 0;
	const double rate_in = std::max( double( sr ), 1.0 );                     // SetRates (:1080-1090)
	double fracpos = 0.0;
	int64_t S = 0, in_frame = 0, out_frame = 0, offset = 0, blocks = 0;
	while( in_frame < n )
		{
		const float slot = std::floor( float( in_frame ) / float( g ) );         // :271, the fp32 quotient
		const int64_t index = int64_t( slot );
		if( index < 0 || index >= count ) { set_error( "repitch: %lld factors are fewer than the loop needs", (long long) count ); return FLANHIP_ERR_INVALID_ARG; }
		const double rate_out = std::max( double( sr ) * double( inv[index] ), 1.0 );
		const double ratio = rate_in / rate_out;
		if( fsize && S < prelude ) S = prelude;                                  // :1226-1237, the first call only
		const double span = ratio * double( g );
		if( !( span < 1.0e15 ) ) { set_error( "repitch: ratio times granularity out of range" ); return FLANHIP_ERR_UNSUPPORTED; }
		const int64_t wanted = std::max<int64_t>( int64_t( span ) + 4 + fsize - S, 0 );      // :1241-1244
		S += wanted;                                                             // :1295
		RpBlock b{};
		b.offset = offset; b.fracpos = fracpos; b.ratio = ratio; b.first_out = out_frame; b.wanted = int32_t( std::min<int64_t>( wanted, INT32_MAX ) );
		b.filtpos = 1.0; b.oversize = 1; b.ideal = 0;
		if( fsize ) wdl_table_shape( rate_in, rate_out, ratio, &b.filtpos, &b.oversize, &b.ideal );
		if( keep ) out->blocks.push_back( b );
		double srcpos = fracpos;
		for( int64_t j = 0; j < g; ++j ) srcpos += ratio;
		const int64_t isrcpos = wdl_hand_over( srcpos, S, b.ideal, b.oversize, &fracpos );      // (ideal is 0 without a table)
		S -= isrcpos;
		offset += isrcpos;
		in_frame += wanted;
		out_frame += g;
		++blocks;
		if( blocks * g > RP_MAX_WORK ) { set_error( "repitch: more than 2^33 output frames" ); return FLANHIP_ERR_UNSUPPORTED; }
		if( blocks > RP_MAX_BLOCKS ) { set_error( "repitch: more than 2^22 blocks (granularity too fine for this length and factor)" ); return FLANHIP_ERR_UNSUPPORTED; }
		}
	*num_blocks = blocks;
	return FLANHIP_OK;
	}

// Runs: consecutive blocks with one table, at most RP_RUN_OUTPUTS output frames, and -- where one block's own window allows it -- a
// stream window that fits the staging buffer.
void rp_runs( const RpPlan & plan, int64_t g, int quality, std::vector<RpRun> * runs )
	{
	const int fsize = quality == FLANHIP_REPITCH_SINC ? RP_TAPS : 0;
	const int64_t max_blocks = std::max<int64_t>( RP_RUN_OUTPUTS / g, 1 );
	auto block_end = [&]( const RpBlock & b ) { return b.offset + int64_t( b.ratio * double( g ) ) + 4 + fsize; };
	size_t i = 0;
	while( i < plan.blocks.size() )
		{
		const RpBlock & a = plan.blocks[i];
		RpRun r{};
		r.first_block = int64_t( i ); r.oversize = a.oversize; r.ideal = a.ideal; r.filtpos = a.filtpos; r.win_start = a.offset;
		int64_t end = block_end( a );
		size_t k = i + 1;
		while( k < plan.blocks.size() && int64_t( k - i ) < max_blocks )
			{
			const RpBlock & b = plan.blocks[k];
			if( !wdl_same_table( a, b ) ) break;
			const int64_t e = std::max( end, block_end( b ) );
			if( e - r.win_start > RP_WINDOW_FLOATS ) break;
			end = e; ++k;
			}
		r.num_blocks = int32_t( k - i );
		r.win_len = end - r.win_start <= RP_WINDOW_FLOATS ? int32_t( end - r.win_start ) : 0;
		runs->push_back( r );
		i = k;
		}
	}

WdlLayout rp_layout( int64_t num_blocks, int64_t num_runs ) { return wdl_layout<RP_TAPS>( sizeof( RpBlock ), num_blocks, sizeof( RpRun ), num_runs ); }

// grid: runs x channel groups of `cpw` channels.  x float[ch][n], out float[ch][out_frames].
__global__ __launch_bounds__( RP_THREADS ) void k_repitch_sinc( const float * __restrict__ x, int64_t ch, int64_t n, int64_t g, int64_t out_frames,
	const RpBlock * __restrict__ blocks, const RpRun * __restrict__ runs, const double * __restrict__ win, int64_t groups, int cpw,
	float * __restrict__ out )
	{
	__shared__ float s_tab[Rp::TABLE_FLOATS];
	__shared__ float s_in[RP_WINDOW_FLOATS];
	__shared__ double s_red[RP_THREADS];
	const int lane = threadIdx.x;
	const int64_t run_index = int64_t( blockIdx.x ) / groups;
	const int64_t c0 = ( int64_t( blockIdx.x ) - run_index * groups ) * cpw;
	const RpRun run = runs[run_index];
	const int oversize = run.oversize;
	wdl_build_table<RP_TAPS>( s_tab, s_red, win + size_t( oversize - 1 ) * Rp::WIN_SLOT, oversize, run.filtpos );

	const int64_t total = int64_t( run.num_blocks ) * g;
	const int64_t c1 = c0 + cpw < ch ? c0 + cpw : ch;
	for( int64_t c = c0; c < c1; ++c )
		{
		const float * xc = x + c * n;
		__syncthreads();                                                         // the table is whole; the last channel's reads of s_in are done
		for( int i = lane; i < run.win_len; i += RP_THREADS ) s_in[i] = wdl_stream<RP_TAPS>( xc, n, run.win_start + i );
		__syncthreads();
		for( int64_t t = lane; t < total; t += RP_THREADS )
			{
			const int64_t bi = t / g, j = t - bi * g;
			const RpBlock b = blocks[run.first_block + bi];
			const int64_t frame = b.first_out + j;
			if( frame >= out_frames ) continue;
			const double srcpos = fma( double( j ), b.ratio, b.fracpos );
			out[c * out_frames + frame] = wdl_sample<RP_TAPS>( s_tab, s_in, run.win_start, run.win_len, xc, n, b.offset, srcpos, oversize, run.ideal );
			}
		}
	}

// SetMode( false, 0, false ): point sampling (:1418-1459).  One thread per ( channel, block, j ).
__global__ __launch_bounds__( RP_THREADS ) void k_repitch_point( const float * __restrict__ x, int64_t ch, int64_t n, int64_t g, int64_t out_frames,
	const RpBlock * __restrict__ blocks, int64_t num_blocks, float * __restrict__ out )
	{
	const int64_t per_channel = num_blocks * g;
	const int64_t count = per_channel * ch;
	for( int64_t t = int64_t( blockIdx.x ) * RP_THREADS + threadIdx.x; t < count; t += int64_t( gridDim.x ) * RP_THREADS )
		{
		const int64_t c = t / per_channel, r = t - c * per_channel;
		const int64_t bi = r / g, j = r - bi * g;
		const RpBlock b = blocks[bi];
		const int64_t frame = b.first_out + j;
		if( frame >= out_frames ) continue;
		const double srcpos = fma( double( j ), b.ratio, b.fracpos );
		out[c * out_frames + frame] = wdl_stream( x + c * n, n, 0, b.offset + int64_t( srcpos ) );
		}
	}

// output frames no block reaches stay 0 (:254-256, the output is constructed zeroed)
__global__ __launch_bounds__( RP_THREADS ) void k_repitch_tail( float * __restrict__ out, int64_t ch, int64_t out_frames, int64_t reached )
	{
	const int64_t tail = out_frames - reached;
	const int64_t count = tail * ch;
	for( int64_t t = int64_t( blockIdx.x ) * RP_THREADS + threadIdx.x; t < count; t += int64_t( gridDim.x ) * RP_THREADS )
		{
		const int64_t c = t / tail;
		out[c * out_frames + reached + ( t - c * tail )] = 0.0f;
		}
	}

int rp_check( const void * x, int64_t ch, int64_t n, float sr, const float * inv, int64_t count, int64_t g, int quality, const void * out )
	{
	FLANHIP_REQUIRE( x && inv && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0 && count > 0 && g > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( quality == FLANHIP_REPITCH_SINC || quality == FLANHIP_REPITCH_LINEAR || quality == FLANHIP_REPITCH_UNINTERPOLATED,
		FLANHIP_ERR_INVALID_ARG, "unknown quality" );
	FLANHIP_REQUIRE( quality != FLANHIP_REPITCH_LINEAR, FLANHIP_ERR_UNSUPPORTED,
		"the Linear quality (a time-varying biquad across the whole stream, WDL/resample.cpp:1276-1292) is not built" );
	FLANHIP_REQUIRE( n <= RP_MAX_FRAMES && g <= RP_MAX_FRAMES && ch <= ( 1 << 20 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// the plan, its runs and the checks every entry point shares; out_frames 0 is a refusal (nothing to write)
int rp_prepare( int64_t ch, int64_t n, float sr, const float * inv, int64_t count, int64_t g, int quality, RpPlan * plan, std::vector<RpRun> * runs )
	{
	int64_t num_blocks = 0;
	if( int rc = rp_plan( n, sr, inv, count, g, quality, true, plan, &num_blocks ) ) return rc;
	plan->out_frames = rp_out_frames( inv, count, g );
	FLANHIP_REQUIRE( plan->out_frames > 0 && plan->out_frames <= RP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "output length out of range" );
	if( quality == FLANHIP_REPITCH_SINC ) rp_runs( *plan, g, quality, runs );
	return FLANHIP_OK;
	}

// channels per workgroup and channel groups of the sinc launch
int rp_channel_groups( const RpPlan & plan, const std::vector<RpRun> & runs, int64_t g, int64_t ch, int64_t * groups )
	{
	return wdl_channel_groups( int64_t( plan.blocks.size() ) * g, runs.size(), ch, groups );
	}

int launch_repitch( const float * d_x, int64_t ch, int64_t n, int64_t g, int quality, const RpPlan & plan, const std::vector<RpRun> & runs,
	float * d_out, void * d_ws, hipStream_t s )
	{
	const int64_t num_blocks = int64_t( plan.blocks.size() );
	const WdlLayout l = rp_layout( num_blocks, int64_t( runs.size() ) );
	char * ws = static_cast<char*>( d_ws );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.block_off, plan.blocks.data(), sizeof( RpBlock ) * plan.blocks.size(), hipMemcpyHostToDevice, s ) );
	if( !runs.empty() )
		FLANHIP_CHECK( hipMemcpyAsync( ws + l.run_off, runs.data(), sizeof( RpRun ) * runs.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );                                  // the host vectors may go once the copies have read them
	const RpBlock * d_blocks = (const RpBlock*) ( ws + l.block_off );
	const int64_t reached = std::min( num_blocks * g, plan.out_frames );
	if( reached < plan.out_frames )
		{
		const int64_t count = ( plan.out_frames - reached ) * ch;
		const int64_t grid = std::min<int64_t>( ( count + RP_THREADS - 1 ) / RP_THREADS, 8192 );
		if( int rc = launch_kernel( "repitch", k_repitch_tail, grid, RP_THREADS, 0, s, d_out, ch, plan.out_frames, reached ) ) return rc;
		}
	if( quality == FLANHIP_REPITCH_UNINTERPOLATED )
		{
		const int64_t count = num_blocks * g * ch;
		const int64_t grid = std::min<int64_t>( ( count + RP_THREADS - 1 ) / RP_THREADS, 65536 );
		return launch_kernel( "repitch", k_repitch_point, grid, RP_THREADS, 0, s, d_x, ch, n, g, plan.out_frames, d_blocks, num_blocks, d_out );
		}
	const double * d_win = nullptr;
	if( int rc = wdl_window<RP_TAPS>( "repitch", d_ws, l, runs, s, &d_win ) ) return rc;
	int64_t groups = 0;
	const int cpw = rp_channel_groups( plan, runs, g, ch, &groups );
	return launch_kernel( "repitch", k_repitch_sinc, int64_t( runs.size() ) * groups, RP_THREADS, 0, s, d_x, ch, n, g, plan.out_frames, d_blocks,
		(const RpRun*) ( ws + l.run_off ), d_win, groups, cpw, d_out );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_audio_repitch_out_frames( const float * inv_factors, int64_t count, int64_t granularity_frames )
	{
	if( !inv_factors || count <= 0 || granularity_frames <= 0 ) return 0;
	return rp_out_frames( inv_factors, count, granularity_frames );
	}

int64_t flanhip_audio_repitch_plan( int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count, int64_t granularity_frames,
	int quality, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize, int32_t * ideal,
	int64_t * first_out, int32_t * wanted, int64_t * out_frames )
	{
	static const float dummy = 0.0f;
	if( int rc = rp_check( &dummy, 1, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &dummy ) ) return rc;
	RpPlan plan;
	int64_t num_blocks = 0;
	if( int rc = rp_plan( num_frames, sample_rate, inv_factors, count, granularity_frames, quality, capacity > 0, &plan, &num_blocks ) ) return rc;
	if( out_frames ) *out_frames = rp_out_frames( inv_factors, count, granularity_frames );
	return wdl_export_plan( plan.blocks, num_blocks, capacity, offsets, fracpos, ratio, filtpos, oversize, ideal, first_out,
		[&]( int64_t i, const RpBlock & b ) { if( wanted ) wanted[i] = b.wanted; } );
	}

int64_t flanhip_audio_repitch_runs( int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count, int64_t granularity_frames,
	int quality, int64_t num_channels, int64_t capacity, int64_t * first_block, int32_t * num_blocks, int64_t * win_start, int32_t * win_len,
	int32_t * channels_per_group, int64_t * groups )
	{
	static const float dummy = 0.0f;
	if( int rc = rp_check( &dummy, num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &dummy ) ) return rc;
	RpPlan plan;
	std::vector<RpRun> runs;
	if( int rc = rp_prepare( num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &plan, &runs ) ) return rc;
	int64_t grp = 0;
	const int cpw = runs.empty() ? 0 : rp_channel_groups( plan, runs, granularity_frames, num_channels, &grp );     // (no runs: the point kernel has no groups)
	if( channels_per_group ) *channels_per_group = cpw;
	if( groups ) *groups = grp;
	const int64_t fill = std::min<int64_t>( std::max<int64_t>( capacity, 0 ), int64_t( runs.size() ) );
	for( int64_t i = 0; i < fill; ++i )
		{
		const RpRun & r = runs[size_t( i )];
		if( first_block ) first_block[i] = r.first_block;
		if( num_blocks ) num_blocks[i] = r.num_blocks;
		if( win_start ) win_start[i] = r.win_start;
		if( win_len ) win_len[i] = r.win_len;
		}
	return int64_t( runs.size() );
	}

size_t flanhip_audio_repitch_workspace_bytes( int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count,
	int64_t granularity_frames, int quality )
	{
	static const float dummy = 0.0f;
	if( rp_check( &dummy, 1, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &dummy ) ) return 0;
	RpPlan plan;
	std::vector<RpRun> runs;
	if( rp_prepare( 1, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &plan, &runs ) ) return 0;
	return rp_layout( int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total;
	}

int flanhip_audio_repitch_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate, const float * inv_factors,
	int64_t count, int64_t granularity_frames, int quality, float * d_out, void * d_workspace, void * stream )
	{
	if( int rc = rp_check( d_audio, num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, d_out ) ) return rc;
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	RpPlan plan;
	std::vector<RpRun> runs;
	if( int rc = rp_prepare( num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &plan, &runs ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_repitch( d_audio, num_channels, num_frames, granularity_frames, quality, plan, runs, d_out, d_workspace, (hipStream_t) stream );
	}

int flanhip_audio_repitch( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate, const float * inv_factors,
	int64_t count, int64_t granularity_frames, int quality, float * out, volatile int * cancel )
	{
	if( int rc = rp_check( audio, num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, out ) ) return rc;
	RpPlan plan;
	std::vector<RpRun> runs;
	if( int rc = rp_prepare( num_channels, num_frames, sample_rate, inv_factors, count, granularity_frames, quality, &plan, &runs ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_x = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( audio, sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), &d_x ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( plan.out_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( rp_layout( int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_repitch( d_x, num_channels, num_frames, granularity_frames, quality, plan, runs, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
