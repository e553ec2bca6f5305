// spatial.hip -- Audio/AudioSpatial.cpp: Audio::stereo_spatialize (:88-281), pan / pan_in_place / widen (:9-45), and the channel plumbing
// they rest on: convert_to_stereo / convert_to_mono (Audio/AudioConversions.cpp:58-104), combine_channels / split_channels
// (Audio/AudioChannels.cpp).  DESIGN.md section 4.20.
//
// stereo_spatialize renders a mono source that moves in the plane once per ear: level difference (head_ild, :116-131), distance
// falloff (:104-114) and an interaural delay that follows the distance and so produces Doppler (head_itd, :135-221).
//   k_spat_ear         both ears of a frame in one pass: the sinusoidal blend of the input with its 500 Hz low-pass, times 1 / distance
//   k_spat_delay       head_itd for a source that stands still: a pure delay (:139-153)
//   k_wdl_window<32>   the Blackman-Harris factor of every table entry, per oversize in use, in fp64 (once per call)
//   k_spat_itd         head_itd for a moving source.  The reference feeds one WDL_Resampler 32 input frames at a time in FEED mode
//                      (SetFeedMode( true ), SetMode( true, 0, true, 32 )) with a rate that changes every block; what comes out of a block
//                      depends on the data.  Between blocks the resampler carries two numbers (the fractional read position and how many
//                      samples stay buffered), which a host loop reproduces exactly in fp64 (sp_plan: one addition per output frame);
//                      after that every output sample is an independent 32-tap sum (two, blended, unless the rates are "ideal") over
//                      a window of one continuous stream: 15 zeros, the input, zeros.  One workgroup per run: consecutive blocks that
//                      share a coefficient table, or a slice of one block whose output count exceeds a run's.
//   k_pan, k_to_stereo, k_to_mono, k_copy_rows    one pass each, 16 bytes per access where the rows' alignment allows
// Every sum runs in a fixed order and nothing is atomic, so two runs agree bit for bit.
#include "wdl_sinc.h"

namespace flanhip {

namespace {

constexpr int SP_G = 32;                       // granularity_frames (:137): input frames per block
constexpr int SP_TAPS = 32;                    // SetMode( true, 0, true, 32 ): m_sincsize
using Sp = WdlSinc<SP_TAPS>;                   // the resampler itself is wdl_sinc.h's, shared with repitch.hip
constexpr int SP_THREADS = WDL_THREADS;
constexpr int SP_RUN_BLOCKS = 64;              // blocks of a run at most: their records and the prefix of their counts sit in LDS
constexpr int SP_RUN_OUTPUTS = 2048;           // output frames per run at most (8 per thread)
constexpr int SP_WINDOW_FLOATS = SP_RUN_BLOCKS * SP_G + 128;   // the staged stream window of a run; what lies outside is read from global memory
constexpr int64_t SP_MAX_FRAMES = int64_t( 1 ) << 31;   // the reference's Frame is an int
constexpr int64_t SP_MAX_BLOCKS = int64_t( 1 ) << 22;   // blocks a call may have per ear: 56 bytes of record each on the host and in the workspace
constexpr int64_t SP_MAX_WORK = int64_t( 1 ) << 33;     // additions the host loop accepts per ear
constexpr int SP_MAX_EARS = 2;
constexpr double SP_MIN_STRETCH = 1.0 / 16.0, SP_MAX_STRETCH = 1024.0;     // the method itself stays within ( 1 / 2, 343 ]

struct SpBlock                                 // one call of ResamplePrepare / ResampleOut
	{
	int64_t offset;                            // stream index of the buffer's first sample
	double fracpos;                            // srcpos of the block's first output sample, relative to offset
	double ratio;
	double filtpos;
	int64_t first_out;                         // the block's first output frame
	int32_t oversize, ideal;
	int32_t count;                             // output frames the block delivers
	int32_t buffered;                          // S: samples in the buffer while the block runs
	};

struct SpRun                                   // one workgroup
	{
	int64_t first_block;                       // index into the ear's records
	int32_t num_blocks, oversize;
	double filtpos;
	int64_t win_start;                         // stream index of the first staged sample
	int32_t win_len, ideal;                    // staged samples
	int64_t first_out;                         // the run's first output frame
	int32_t first_j, count;                    // a run of ONE block may be a slice of it: outputs [first_j, first_j + count) of the block
	int32_t ear, pad;
	};
static_assert( sizeof( SpBlock ) == 56 && sizeof( SpRun ) == 64, "the device reads these records as the host lays them out" );

struct SpPlan
	{
	std::vector<SpBlock> blocks;
	int64_t total_out = 0;                     // output frames the blocks deliver together
	};

int64_t sp_count( int64_t n ) { return ( n + SP_G - 1 ) / SP_G; }              // blocks of the loop of :194, and stretches.size() (:160-170)

// :159-186: the stretches (when asked for) and the output length from the distances at frames 0, 32, 64, ...
int64_t sp_out_frames( int64_t n, float sr, const double * dist, int64_t count, double * stretches )
	{
	const float sound_mps = 343;
	float max_needed_length = 0;                                                 // a Second
	double previous = dist[0];
	if( stretches ) stretches[0] = 1.0 / ( 1.0 - 0.0 / SP_G / double( sound_mps ) * sr );
	for( int64_t k = 1; k < count; ++k )
		{
		const int64_t frame = k * SP_G;
		const double current = dist[k];
		const double change = current - previous;
		previous = current;
		if( stretches ) stretches[k] = 1.0 / ( 1.0 - change / SP_G / double( sound_mps ) * sr );      // :185
		const float receive = float( ( float( frame + SP_G ) / sr ) + current / sound_mps );           // :168, float + double, stored in a float
		if( max_needed_length < receive ) max_needed_length = receive;
		}
	const float frames = std::ceil( max_needed_length * sr );                     // :174
	if( !( frames > 0.0f ) ) return 0;
	return frames >= 2147483648.0f ? INT64_MAX : int64_t( frames );
	}

// The block loop of :194-218 with the state of ResamplePrepare (WDL/resample.cpp:1218-1265, feed mode: 32 frames go in) and ResampleOut
// (:1295, :1313, :1339-1361, :1558-1566), in fp64 with the reference's own chain of srcpos += ratio.  keep: store the records (else count
// only).  FLANHIP_OK, or why the loop cannot run.
int sp_plan( int64_t n, float sr, const double * stretches, int64_t count, bool keep, SpPlan * out, int64_t * num_blocks )
	{
	const double rate_in = std::max( double( sr ), 1.0 );                         // SetRates (:1080-1090)
	double fracpos = 0.0;
	int64_t S = 0, offset = 0, out_frame = 0, work = 0;
	if( count != sp_count( n ) ) { set_error( "spatial_itd: %lld stretches, the loop needs %lld", (long long) count, (long long) sp_count( n ) ); return FLANHIP_ERR_INVALID_ARG; }
	if( count > SP_MAX_BLOCKS ) { set_error( "spatial_itd: more than 2^22 blocks" ); return FLANHIP_ERR_UNSUPPORTED; }
	for( int64_t b = 0; b < count; ++b )
		{
		const double stretch = stretches[b];
		if( !( stretch >= SP_MIN_STRETCH && stretch <= SP_MAX_STRETCH ) ) { set_error( "spatial_itd: stretch %g of block %lld is outside [1/16, 1024]", stretch, (long long) b ); return FLANHIP_ERR_INVALID_ARG; }
		const double rate_out = std::max( double( sr ) * stretch, 1.0 );
		const double ratio = rate_in / rate_out;
		if( S < Sp::PRELUDE )                                                     // :1226-1237: the first call only
			{
			if( b ) { set_error( "spatial_itd: the buffer ran below the prelude in block %lld", (long long) b ); return FLANHIP_ERR_UNSUPPORTED; }
			S = Sp::PRELUDE;
			}
		S += SP_G;                                                               // :1242, :1295
		SpBlock r{};
		r.offset = offset; r.fracpos = fracpos; r.ratio = ratio; r.first_out = out_frame; r.buffered = int32_t( S );
		wdl_table_shape( rate_in, rate_out, ratio, &r.filtpos, &r.oversize, &r.ideal );
		int64_t ns = int64_t( std::ceil( SP_G * stretch ) );                     // :210
		const int64_t limit = S - SP_TAPS - 1;                                   // ipos >= filtlen - 1 ends the block (:1343)
		double srcpos = fracpos;
		int64_t delivered = 0;
		while( ns-- && int64_t( srcpos ) < limit ) { srcpos += ratio; ++delivered; }
		r.count = int32_t( delivered );
		if( keep ) out->blocks.push_back( r );
		const int64_t isrcpos = wdl_hand_over( srcpos, S, r.ideal, r.oversize, &fracpos );
		S -= isrcpos;
		offset += isrcpos;
		out_frame += delivered;
		work += delivered + 1;
		if( work > SP_MAX_WORK ) { set_error( "spatial_itd: more than 2^33 output frames" ); return FLANHIP_ERR_UNSUPPORTED; }
		}
	if( out ) out->total_out = out_frame;
	*num_blocks = count;
	return FLANHIP_OK;
	}

// Runs of one ear: consecutive blocks with one table, at most SP_RUN_BLOCKS of them and SP_RUN_OUTPUTS output frames, whose stream window
// fits the staging buffer; a block with more outputs than that is cut into slices, each a run of its own.  Output frames from `keep` on
// are dropped (:213-215): no run is made for them.
void sp_runs( const SpPlan & plan, int ear, int64_t keep, std::vector<SpRun> * runs )
	{
	size_t i = 0;
	while( i < plan.blocks.size() )
		{
		const SpBlock & a = plan.blocks[i];
		if( a.first_out >= keep ) break;
		SpRun r{};
		r.first_block = int64_t( i ); r.oversize = a.oversize; r.ideal = a.ideal; r.filtpos = a.filtpos; r.win_start = a.offset; r.ear = ear;
		r.first_out = a.first_out;
		if( a.count > SP_RUN_OUTPUTS )
			{
			r.num_blocks = 1;
			r.win_len = int32_t( std::min<int64_t>( a.buffered, SP_WINDOW_FLOATS ) );
			for( int32_t j = 0; j < a.count && a.first_out + j < keep; j += SP_RUN_OUTPUTS )
				{
				r.first_j = j; r.count = std::min( a.count - j, SP_RUN_OUTPUTS ); r.first_out = a.first_out + j;
				runs->push_back( r );
				}
			++i;
			continue;
			}
		int64_t end = a.offset + a.buffered, total = a.count;
		size_t k = i + 1;
		while( k < plan.blocks.size() && int64_t( k - i ) < SP_RUN_BLOCKS )
			{
			const SpBlock & b = plan.blocks[k];
			if( !wdl_same_table( a, b ) || b.first_out >= keep ) break;
			if( total + b.count > SP_RUN_OUTPUTS ) break;
			const int64_t e = std::max( end, b.offset + b.buffered );
			if( e - r.win_start > SP_WINDOW_FLOATS ) break;
			end = e; total += b.count; ++k;
			}
		r.num_blocks = int32_t( k - i );
		r.first_j = 0; r.count = int32_t( total );
		r.win_len = int32_t( std::min<int64_t>( end - r.win_start, SP_WINDOW_FLOATS ) );
		if( total > 0 ) runs->push_back( r );
		i = k;
		}
	}

// the workspace: the window factors, then every ear's block records one after the other, then all runs (room for one where there is none)
WdlLayout sp_layout( int64_t num_blocks, int64_t num_runs )
	{
	return wdl_layout<SP_TAPS>( sizeof( SpBlock ), num_blocks, sizeof( SpRun ), std::max<int64_t>( num_runs, 1 ) );
	}

struct SpEars                                  // per ear: where its block records start, and how many output frames it keeps
	{
	int64_t block_base[SP_MAX_EARS];
	int64_t out_frames[SP_MAX_EARS];
	};

// grid: all ears' runs, the ear outermost.  x float[ears][n], out float[ears][out_stride].
__global__ __launch_bounds__( SP_THREADS ) void k_spat_itd( const float * __restrict__ x, int64_t n, SpEars ears, int64_t out_stride,
	const SpBlock * __restrict__ blocks, const SpRun * __restrict__ runs, const double * __restrict__ win, float * __restrict__ out )
	{
	__shared__ float s_tab[Sp::TABLE_FLOATS];
	__shared__ float s_in[SP_WINDOW_FLOATS];
	__shared__ double s_red[SP_THREADS];
	__shared__ SpBlock s_blk[SP_RUN_BLOCKS];
	__shared__ int s_first[SP_RUN_BLOCKS + 1];                                   // the run's prefix of output counts
	const int lane = threadIdx.x;
	const SpRun run = runs[blockIdx.x];
	const int ear = run.ear;
	const int oversize = run.oversize;
	const float * xe = x + int64_t( ear ) * n;
	const SpBlock * eb = blocks + ears.block_base[ear] + run.first_block;
	const int64_t out_frames = ears.out_frames[ear];

	if( lane < run.num_blocks )
		{
		const SpBlock b = eb[lane];
		s_blk[lane] = b;
		s_first[lane] = int( b.first_out - eb[0].first_out );
		}
	if( lane == 0 ) s_first[run.num_blocks] = run.first_j + run.count;           // (first_j is 0 unless the run is a slice of one block)
	for( int i = lane; i < run.win_len; i += SP_THREADS ) s_in[i] = wdl_stream<SP_TAPS>( xe, n, run.win_start + i );

	wdl_build_table<SP_TAPS>( s_tab, s_red, win + size_t( oversize - 1 ) * Sp::WIN_SLOT, oversize, run.filtpos );
	__syncthreads();

	for( int t = lane; t < run.count; t += SP_THREADS )
		{
		// the block output t of the run belongs to: the last one whose first output is not past it (blocks may deliver nothing)
		const int at = run.first_j + t;
		int lo = 0, hi = run.num_blocks;
		while( hi - lo > 1 )
			{
			const int mid = ( lo + hi ) >> 1;
			if( s_first[mid] <= at ) lo = mid; else hi = mid;
			}
		const SpBlock & b = s_blk[lo];
		const int j = at - s_first[lo];
		const int64_t frame = b.first_out + j;
		if( frame >= out_frames ) continue;                                      // :213-215
		const double srcpos = fma( double( j ), b.ratio, b.fracpos );
		out[int64_t( ear ) * out_stride + frame] = wdl_sample<SP_TAPS>( s_tab, s_in, run.win_start, run.win_len, xe, n, b.offset, srcpos, oversize, run.ideal );
		}
	}

// output frames no block reaches stay 0 (:176-177), and so does the row's padding up to out_stride
__global__ __launch_bounds__( SP_THREADS ) void k_spat_tail( float * __restrict__ out, int64_t out_stride, SpEars reached )
	{
	const int ear = blockIdx.y;
	float * row = out + int64_t( ear ) * out_stride;
	for( int64_t t = reached.out_frames[ear] + int64_t( blockIdx.x ) * SP_THREADS + threadIdx.x; t < out_stride; t += int64_t( gridDim.x ) * SP_THREADS ) row[t] = 0.0f;
	}

// :139-153: out[ Frame( frame + delay ) ] = in[ frame ], the index formed in fp32 as the reference forms it.  The index does not fall as the
// frame rises, and where two frames share one the reference's loop leaves the later: a frame writes unless the next one lands on its index
struct SpDelays { float delay[SP_MAX_EARS]; int64_t out_frames[SP_MAX_EARS]; };
__global__ __launch_bounds__( SP_THREADS ) void k_spat_delay( const float * __restrict__ x, int64_t n, SpDelays d, int64_t out_stride, float * __restrict__ out )
	{
	const int ear = blockIdx.y;
	const int64_t f = int64_t( blockIdx.x ) * SP_THREADS + threadIdx.x;
	if( f >= n ) return;
	const int64_t at = int64_t( __fadd_rn( float( f ), d.delay[ear] ) );
	if( at < 0 || at >= d.out_frames[ear] ) return;
	if( f + 1 < n && int64_t( __fadd_rn( float( f + 1 ), d.delay[ear] ) ) == at ) return;
	out[int64_t( ear ) * out_stride + at] = x[int64_t( ear ) * n + f];
	}

// head_ild (:116-131) and falloff (:104-114) for the ears asked for, one frame per thread.  The weight and the distance of frame f are read
// at index int( ( f * ( 1.0f / sr ) ) * sr ), formed in fp32: to_time_function (FunctionSample.h:130-133) and time_to_frame inside callables
// that are sampled at f * ( 1.0f / sr ).  For some f that is f - 1.
struct SpEarArgs
	{
	const float * x, * lp;                     // the input and its 500 Hz low-pass, float[n]
	const double * pos;                        // double[n][2], or null for the constant ( px, py )
	double px, py;
	int64_t n;
	float sr, inv_sr, half_width;              // half_width: head_width / 2.0f
	int first, ears;                           // the ears written: first ... first + ears - 1 (0 left, 1 right) to rows 0 ...
	float * out;                               // float[ears][n]
	};
__global__ __launch_bounds__( SP_THREADS ) void k_spat_ear( SpEarArgs a )
	{
	const int64_t f = int64_t( blockIdx.x ) * SP_THREADS + threadIdx.x;
	if( f >= a.n ) return;
	int64_t q = int64_t( __fmul_rn( __fmul_rn( float( f ), a.inv_sr ), a.sr ) );
	q = q < 0 ? 0 : q > a.n - 1 ? a.n - 1 : q;
	const double px = a.pos ? a.pos[2 * q] : a.px, py = a.pos ? a.pos[2 * q + 1] : a.py;
	const float x = a.x[f], lp = a.lp[f];
	const float pi = 3.14159274101257324f;                                       // acos( -1.0f )
	const float pi2 = pi * 2.0f;
	for( int e = 0; e < a.ears; ++e )
		{
		const bool left = a.first + e == 0;
		const double ear_y = double( left ? a.half_width : -a.half_width );     // :261
		const double rx = px - 0.0, ry = py - ear_y;                             // :263
		const float direct = ( left ? 75.0f : -75.0f ) * pi2 / 360.0f;           // :276-277
		const float angle = atan2f( float( ry ), float( rx ) ) - direct;        // :120-121, std::arg of a complex<float>
		const float mix = 0.5f + 0.5f * cosf( angle );                           // :122
		const float dist = float( sqrt( rx * rx + ry * ry ) );                   // :111, vec2d::mag() into a Meter
		const float gain = 1.0f / ( dist + 0.00001f );                           // :112
		const float blended = lp * ( 1.0f - mix ) + x * mix;                     // :129-130 (every operation rounded: no contraction in this file)
		a.out[int64_t( e ) * a.n + f] = blended * gain;
		}
	}

// ---- pan, the conversions, the channel copies -------------------------------------------------------------------------------------------
typedef float f4 __attribute__(( ext_vector_type( 4 ) ));

// four frames from f on (the first `valid` of them): one 16-byte access where VEC says the rows allow it and the quad is whole
template<bool VEC>
__device__ __forceinline__ void sp_load4( const float * p, int64_t f, int valid, float ( &v )[4] )
	{
	if( VEC && valid == 4 )
		{
		const f4 q = *reinterpret_cast<const f4*>( p + f );
		v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
		return;
		}
	#pragma unroll
	for( int k = 0; k < 4; ++k ) v[k] = k < valid ? p[f + k] : 0.0f;
	}
template<bool VEC>
__device__ __forceinline__ void sp_store4( float * p, int64_t f, int valid, const float ( &v )[4] )
	{
	if( VEC && valid == 4 )
		{
		const f4 q = { v[0], v[1], v[2], v[3] };
		*reinterpret_cast<f4*>( p + f ) = q;
		return;
		}
	#pragma unroll
	for( int k = 0; k < 4; ++k ) if( k < valid ) p[f + k] = v[k];
	}
inline int64_t sp_quads( int64_t n ) { return ( n + 3 ) / 4; }

// Interpolator::sine2 (Utility/Interpolator.cpp:85-91) as the reference's compiler resolves it: pi / 4.0f * x is fp32, the unqualified sin is
// the DOUBLE one, the fp32 sqrt2 is promoted to it and the product is rounded once when the std::function returns a float
__device__ __forceinline__ float sp_sine2( float x )
	{
	const float pi = 3.14159274101257324f, sqrt2 = 1.41421354f;
	return float( double( sqrt2 ) * sin( double( pi / 4.0f * x ) ) );
	}

// Audio::pan_in_place (:21-40): x[0][f] *= sine2( p ), x[1][f] *= sine2( 1 - p ), p = pan[f] / 2.0f + 0.5f.  in / out: float[2][n]
template<bool VEC>
__global__ __launch_bounds__( 256 ) void k_pan( const float * in, int64_t n, const float * __restrict__ pan, float pan_c, float * out )
	{
	const int64_t f = ( int64_t( blockIdx.x ) * 256 + threadIdx.x ) * 4;
	if( f >= n ) return;
	const int valid = int( std::min<int64_t>( n - f, 4 ) );
	float p[4] = { pan_c, pan_c, pan_c, pan_c }, l[4], r[4];
	if( pan ) sp_load4<VEC>( pan, f, valid, p );
	sp_load4<VEC>( in, f, valid, l );
	sp_load4<VEC>( in + n, f, valid, r );
	#pragma unroll
	for( int k = 0; k < 4; ++k )
		{
		const float q = p[k] / 2.0f + 0.5f;                                      // :33
		l[k] = l[k] * sp_sine2( q );
		r[k] = r[k] * sp_sine2( 1.0f - q );                                      // :34
		}
	sp_store4<VEC>( out, f, valid, l );
	sp_store4<VEC>( out + n, f, valid, r );
	}

// Audio::convert_to_stereo of a mono input (AudioConversions.cpp:68-77): both channels s / sqrt( 2.0f )
template<bool VEC>
__global__ __launch_bounds__( 256 ) void k_to_stereo( const float * __restrict__ in, int64_t n, float * __restrict__ out )
	{
	const int64_t f = ( int64_t( blockIdx.x ) * 256 + threadIdx.x ) * 4;
	if( f >= n ) return;
	const int valid = int( std::min<int64_t>( n - f, 4 ) );
	float v[4];
	sp_load4<VEC>( in, f, valid, v );
	#pragma unroll
	for( int k = 0; k < 4; ++k ) v[k] = v[k] / 1.41421354f;
	sp_store4<VEC>( out, f, valid, v );
	sp_store4<VEC>( out + n, f, valid, v );
	}

// Audio::convert_to_mono (:87-104): the channels added in order from 0.0f, the sum divided by their number
template<bool VEC>
__global__ __launch_bounds__( 256 ) void k_to_mono( const float * __restrict__ in, int64_t ch, int64_t n, float * __restrict__ out )
	{
	const int64_t f = ( int64_t( blockIdx.x ) * 256 + threadIdx.x ) * 4;
	if( f >= n ) return;
	const int valid = int( std::min<int64_t>( n - f, 4 ) );
	float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
	for( int64_t c = 0; c < ch; ++c )
		{
		float v[4];
		sp_load4<VEC>( in + c * n, f, valid, v );
		#pragma unroll
		for( int k = 0; k < 4; ++k ) acc[k] = acc[k] + v[k];
		}
	const float count = float( ch );
	#pragma unroll
	for( int k = 0; k < 4; ++k ) acc[k] = acc[k] / count;
	sp_store4<VEC>( out, f, valid, acc );
	}

// rows of src_frames floats, src_stride apart, to rows dst_stride apart; each destination row is dst_frames long and the rest of it zero
// (Audio::combine_channels, AudioChannels.cpp:47-59; split_channels, :13-29).  grid.y: the row
template<bool VEC>
__global__ __launch_bounds__( 256 ) void k_copy_rows( const float * __restrict__ src, int64_t src_stride, int64_t src_frames,
	float * __restrict__ dst, int64_t dst_stride, int64_t dst_frames )
	{
	const int64_t f = ( int64_t( blockIdx.x ) * 256 + threadIdx.x ) * 4;
	if( f >= dst_frames ) return;
	const int64_t row = blockIdx.y;
	const int valid = int( std::min<int64_t>( dst_frames - f, 4 ) );
	const int have = int( std::clamp<int64_t>( src_frames - f, 0, 4 ) );
	float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
	if( have ) sp_load4<VEC>( src + row * src_stride, f, have, v );
	sp_store4<VEC>( dst + row * dst_stride, f, valid, v );
	}

// ---- checks and launchers -------------------------------------------------------------------------------------------------------------
int sp_check_itd( const void * x, int64_t ears, int64_t n, float sr, const double * stretches, int64_t count, const int64_t * out_frames,
	int64_t out_stride, const void * out )
	{
	FLANHIP_REQUIRE( x && stretches && out_frames && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ears >= 1 && ears <= SP_MAX_EARS, FLANHIP_ERR_INVALID_ARG, "one or two ears" );
	FLANHIP_REQUIRE( n > 0 && count > 0 && out_stride > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( n <= SP_MAX_FRAMES && out_stride <= SP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	for( int64_t e = 0; e < ears; ++e )
		FLANHIP_REQUIRE( out_frames[e] >= 0 && out_frames[e] <= out_stride, FLANHIP_ERR_INVALID_ARG, "an ear's output length is outside [0, out_stride]" );
	return FLANHIP_OK;
	}

struct SpPrepared
	{
	SpPlan plan[SP_MAX_EARS];
	std::vector<SpRun> runs;
	int64_t num_blocks = 0;
	};

// out_frames: what every ear keeps, or null for all that is delivered (the workspace is sized for that)
int sp_prepare( int64_t ears, int64_t n, float sr, const double * stretches, int64_t count, const int64_t * out_frames, SpPrepared * p )
	{
	for( int64_t e = 0; e < ears; ++e )
		{
		int64_t blocks = 0;
		if( int rc = sp_plan( n, sr, stretches + e * count, count, true, &p->plan[e], &blocks ) ) return rc;
		sp_runs( p->plan[e], int( e ), out_frames ? out_frames[e] : INT64_MAX, &p->runs );
		p->num_blocks += blocks;
		}
	return FLANHIP_OK;
	}

int launch_itd( const float * d_x, int64_t ears, int64_t n, const int64_t * out_frames, int64_t out_stride, const SpPrepared & p,
	float * d_out, void * d_ws, hipStream_t s )
	{
	const WdlLayout l = sp_layout( p.num_blocks, int64_t( p.runs.size() ) );
	char * ws = static_cast<char*>( d_ws );
	SpEars at{}, reached{};
	int64_t base = 0;
	for( int64_t e = 0; e < ears; ++e )
		{
		const std::vector<SpBlock> & b = p.plan[e].blocks;
		FLANHIP_CHECK( hipMemcpyAsync( ws + l.block_off + sizeof( SpBlock ) * size_t( base ), b.data(), sizeof( SpBlock ) * b.size(), hipMemcpyHostToDevice, s ) );
		at.block_base[e] = base; at.out_frames[e] = out_frames[e];
		reached.out_frames[e] = std::min( p.plan[e].total_out, out_frames[e] );
		base += int64_t( b.size() );
		}
	if( !p.runs.empty() )
		FLANHIP_CHECK( hipMemcpyAsync( ws + l.run_off, p.runs.data(), sizeof( SpRun ) * p.runs.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );                                  // the host vectors may go once the copies have read them
	int64_t longest_tail = 0;
	for( int64_t e = 0; e < ears; ++e ) longest_tail = std::max( longest_tail, out_stride - reached.out_frames[e] );
	if( longest_tail > 0 )
		{
		const unsigned grid = unsigned( std::min<int64_t>( ( longest_tail + SP_THREADS - 1 ) / SP_THREADS, 4096 ) );
		hipLaunchKernelGGL( k_spat_tail, dim3( grid, unsigned( ears ) ), dim3( SP_THREADS ), 0, s, d_out, out_stride, reached );
		FLANHIP_CHECK( hipGetLastError() );
		}
	if( p.runs.empty() ) return FLANHIP_OK;
	const double * d_win = nullptr;
	if( int rc = wdl_window<SP_TAPS>( "spatial_itd", d_ws, l, p.runs, s, &d_win ) ) return rc;
	return launch_kernel( "spatial_itd", k_spat_itd, int64_t( p.runs.size() ), SP_THREADS, 0, s, d_x, n, at, out_stride,
		(const SpBlock*) ( ws + l.block_off ), (const SpRun*) ( ws + l.run_off ), d_win, d_out );
	}

int sp_check_ear( const void * x, const void * lp, int64_t ch, int64_t n, float sr, float head_width, int ears, const void * out )
	{
	FLANHIP_REQUIRE( x && lp && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch == 1, FLANHIP_ERR_INVALID_ARG, "only mono inputs are spatialized" );
	FLANHIP_REQUIRE( n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( ears == FLANHIP_SPATIAL_LEFT || ears == FLANHIP_SPATIAL_RIGHT || ears == FLANHIP_SPATIAL_BOTH, FLANHIP_ERR_INVALID_ARG, "unknown ear selection" );
	FLANHIP_REQUIRE( head_width == head_width, FLANHIP_ERR_INVALID_ARG, "head width is not a number" );
	FLANHIP_REQUIRE( n <= SP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

int launch_ear( const float * d_x, const float * d_lp, int64_t n, float sr, const double * d_pos, double px, double py, float head_width, int ears,
	float * d_out, hipStream_t s )
	{
	SpEarArgs a{};
	a.x = d_x; a.lp = d_lp; a.pos = d_pos; a.px = px; a.py = py; a.n = n; a.sr = sr; a.inv_sr = 1.0f / sr; a.half_width = head_width / 2.0f;
	a.first = ears == FLANHIP_SPATIAL_RIGHT ? 1 : 0; a.ears = ears == FLANHIP_SPATIAL_BOTH ? 2 : 1; a.out = d_out;
	return launch_kernel( "spatial_ear", k_spat_ear, ( n + SP_THREADS - 1 ) / SP_THREADS, SP_THREADS, 0, s, a );
	}

int sp_check_pan( const void * x, int64_t ch, int64_t n, const void * out )
	{
	FLANHIP_REQUIRE( x && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch == 2, FLANHIP_ERR_INVALID_ARG, "pan works on two channels" );
	FLANHIP_REQUIRE( n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( n <= SP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

int launch_pan( const float * d_x, int64_t n, const float * d_pan, float pan, float * d_out, hipStream_t s )
	{
	const bool vec = n % 4 == 0 && aligned16( d_x ) && aligned16( d_out ) && aligned16( d_pan );
	return scan_pair( vec, [&]( auto V ) { return launch_kernel( "audio_pan", k_pan<V.value>, ( sp_quads( n ) + 255 ) / 256, 256, 0, s, d_x, n, d_pan, pan, d_out ); } );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_spatial_itd_out_frames( int64_t num_frames, float sample_rate, const double * distances, int64_t count, double * stretches )
	{
	FLANHIP_REQUIRE( distances, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && num_frames <= SP_MAX_FRAMES && sample_rate > 0.0f, FLANHIP_ERR_INVALID_ARG, "bad shape" );
	FLANHIP_REQUIRE( count == sp_count( num_frames ), FLANHIP_ERR_INVALID_ARG, "one distance per 32 input frames, the last block included" );
	return sp_out_frames( num_frames, sample_rate, distances, count, stretches );
	}

int64_t flanhip_spatial_itd_plan( int64_t num_frames, float sample_rate, const double * stretches, int64_t count, int64_t capacity,
	int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize, int32_t * ideal, int64_t * first_out,
	int32_t * delivered, int32_t * buffered, int64_t * total_out )
	{
	FLANHIP_REQUIRE( stretches, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && num_frames <= SP_MAX_FRAMES && count > 0 && sample_rate > 0.0f, FLANHIP_ERR_INVALID_ARG, "bad shape" );
	SpPlan plan;
	int64_t num_blocks = 0;
	if( int rc = sp_plan( num_frames, sample_rate, stretches, count, capacity > 0, &plan, &num_blocks ) ) return rc;
	if( total_out ) *total_out = plan.total_out;
	return wdl_export_plan( plan.blocks, num_blocks, capacity, offsets, fracpos, ratio, filtpos, oversize, ideal, first_out,
		[&]( int64_t i, const SpBlock & b ) { if( delivered ) delivered[i] = b.count; if( buffered ) buffered[i] = b.buffered; } );
	}

size_t flanhip_spatial_itd_workspace_bytes( int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches, int64_t count )
	{
	if( !stretches || num_ears < 1 || num_ears > SP_MAX_EARS || num_frames <= 0 || num_frames > SP_MAX_FRAMES || count <= 0 || !( sample_rate > 0.0f ) ) return 0;
	SpPrepared p;
	if( sp_prepare( num_ears, num_frames, sample_rate, stretches, count, nullptr, &p ) ) return 0;
	return sp_layout( p.num_blocks, int64_t( p.runs.size() ) ).total;
	}

int flanhip_spatial_itd_dev( const float * d_audio, int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches,
	int64_t count, const int64_t * out_frames, int64_t out_stride, float * d_out, void * d_workspace, void * stream )
	{
	if( int rc = sp_check_itd( d_audio, num_ears, num_frames, sample_rate, stretches, count, out_frames, out_stride, d_out ) ) return rc;
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	SpPrepared p;
	if( int rc = sp_prepare( num_ears, num_frames, sample_rate, stretches, count, out_frames, &p ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_itd( d_audio, num_ears, num_frames, out_frames, out_stride, p, d_out, d_workspace, (hipStream_t) stream );
	}

int flanhip_spatial_itd( const float * audio, int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches, int64_t count,
	const int64_t * out_frames, int64_t out_stride, float * out, volatile int * cancel )
	{
	if( int rc = sp_check_itd( audio, num_ears, num_frames, sample_rate, stretches, count, out_frames, out_stride, out ) ) return rc;
	SpPrepared p;
	if( int rc = sp_prepare( num_ears, num_frames, sample_rate, stretches, count, out_frames, &p ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_x = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( audio, sizeof( float ) * size_t( num_ears ) * size_t( num_frames ), &d_x ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_ears ) * size_t( out_stride ), &d_out ) ) return rc;
	if( int rc = call.scratch( sp_layout( p.num_blocks, int64_t( p.runs.size() ) ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_itd( d_x, num_ears, num_frames, out_frames, out_stride, p, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_spatial_delay_dev( const float * d_audio, int64_t num_ears, int64_t num_frames, const float * delays, const int64_t * out_frames,
	int64_t out_stride, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_audio && delays && out_frames && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_ears >= 1 && num_ears <= SP_MAX_EARS, FLANHIP_ERR_INVALID_ARG, "one or two ears" );
	FLANHIP_REQUIRE( num_frames > 0 && out_stride > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= SP_MAX_FRAMES && out_stride <= SP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	SpDelays d{};
	for( int64_t e = 0; e < num_ears; ++e )
		{
		FLANHIP_REQUIRE( delays[e] >= 0.0f && delays[e] < 2147483648.0f, FLANHIP_ERR_INVALID_ARG, "a delay is negative, too large or not a number" );
		FLANHIP_REQUIRE( out_frames[e] >= 0 && out_frames[e] <= out_stride, FLANHIP_ERR_INVALID_ARG, "an ear's output length is outside [0, out_stride]" );
		d.delay[e] = delays[e]; d.out_frames[e] = out_frames[e];
		}
	if( int rc = require_device() ) return rc;
	hipStream_t s = (hipStream_t) stream;
	FLANHIP_CHECK( hipMemsetAsync( d_out, 0, sizeof( float ) * size_t( num_ears ) * size_t( out_stride ), s ) );
	hipLaunchKernelGGL( k_spat_delay, dim3( unsigned( ( num_frames + SP_THREADS - 1 ) / SP_THREADS ), unsigned( num_ears ) ), dim3( SP_THREADS ), 0, s,
		d_audio, num_frames, d, out_stride, d_out );
	FLANHIP_CHECK( hipGetLastError() );
	return FLANHIP_OK;
	}

int flanhip_spatial_ear_dev( const float * d_audio, const float * d_lowpassed, int64_t num_channels, int64_t num_frames, float sample_rate,
	const double * d_positions, double position_x, double position_y, float head_width, int ears, float * d_out, void * stream )
	{
	if( int rc = sp_check_ear( d_audio, d_lowpassed, num_channels, num_frames, sample_rate, head_width, ears, d_out ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_ear( d_audio, d_lowpassed, num_frames, sample_rate, d_positions, position_x, position_y, head_width, ears, d_out, (hipStream_t) stream );
	}

int flanhip_spatial_ear( const float * audio, const float * lowpassed, int64_t num_channels, int64_t num_frames, float sample_rate,
	const double * positions, double position_x, double position_y, float head_width, int ears, float * out, volatile int * cancel )
	{
	if( int rc = sp_check_ear( audio, lowpassed, num_channels, num_frames, sample_rate, head_width, ears, out ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t row = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	const float * d_x = nullptr, * d_lp = nullptr; const double * d_pos = nullptr; float * d_out = nullptr;
	if( int rc = call.in( audio, row, &d_x ) ) return rc;
	if( int rc = call.in( lowpassed, row, &d_lp ) ) return rc;
	if( positions ) if( int rc = call.in( positions, sizeof( double ) * 2 * size_t( num_frames ), &d_pos ) ) return rc;
	if( int rc = call.out( out, row * ( ears == FLANHIP_SPATIAL_BOTH ? 2 : 1 ), &d_out ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_ear( d_x, d_lp, num_frames, sample_rate, d_pos, position_x, position_y, head_width, ears, d_out, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_audio_pan_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_pan, float pan, float * d_out, void * stream )
	{
	if( int rc = sp_check_pan( d_audio, num_channels, num_frames, d_out ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_pan( d_audio, num_frames, d_pan, pan, d_out, (hipStream_t) stream );
	}

int flanhip_audio_pan( const float * audio, int64_t num_channels, int64_t num_frames, const float * pan_curve, float pan, float * out, volatile int * cancel )
	{
	if( int rc = sp_check_pan( audio, num_channels, num_frames, out ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t row = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	const float * d_x = nullptr, * d_pan = nullptr; float * d_out = nullptr;
	if( int rc = call.in( audio, 2 * row, &d_x ) ) return rc;
	if( pan_curve ) if( int rc = call.in( pan_curve, row, &d_pan ) ) return rc;
	if( int rc = call.out( out, 2 * row, &d_out ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_pan( d_x, num_frames, d_pan, pan, d_out, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_audio_to_stereo_dev( const float * d_audio, int64_t num_frames, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_audio && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= SP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	if( int rc = require_device() ) return rc;
	const bool vec = num_frames % 4 == 0 && aligned16( d_audio ) && aligned16( d_out );
	return scan_pair( vec, [&]( auto V ) { return launch_kernel( "audio_to_stereo", k_to_stereo<V.value>, ( sp_quads( num_frames ) + 255 ) / 256, 256, 0,
		(hipStream_t) stream, d_audio, num_frames, d_out ); } );
	}

int flanhip_audio_to_mono_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_audio && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_channels > 0 && num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= SP_MAX_FRAMES && num_channels <= ( 1 << 20 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	if( int rc = require_device() ) return rc;
	const bool vec = num_frames % 4 == 0 && aligned16( d_audio ) && aligned16( d_out );
	return scan_pair( vec, [&]( auto V ) { return launch_kernel( "audio_to_mono", k_to_mono<V.value>, ( sp_quads( num_frames ) + 255 ) / 256, 256, 0,
		(hipStream_t) stream, d_audio, num_channels, num_frames, d_out ); } );
	}

int flanhip_audio_copy_rows_dev( const float * d_src, int64_t src_stride, int64_t num_rows, int64_t src_frames, float * d_dst, int64_t dst_stride,
	int64_t dst_frames, void * stream )
	{
	FLANHIP_REQUIRE( d_src && d_dst, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_rows > 0 && src_frames > 0 && dst_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( src_stride >= src_frames && dst_stride >= dst_frames && dst_frames >= src_frames, FLANHIP_ERR_INVALID_ARG,
		"a row is longer than its stride, or the source longer than the destination" );
	FLANHIP_REQUIRE( dst_frames <= SP_MAX_FRAMES && num_rows < 65536, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	if( int rc = require_device() ) return rc;
	const bool vec = src_stride % 4 == 0 && dst_stride % 4 == 0 && aligned16( d_src ) && aligned16( d_dst );
	const dim3 grid( unsigned( ( sp_quads( dst_frames ) + 255 ) / 256 ), unsigned( num_rows ) );
	hipStream_t s = (hipStream_t) stream;
	if( vec ) hipLaunchKernelGGL( k_copy_rows<true>, grid, dim3( 256 ), 0, s, d_src, src_stride, src_frames, d_dst, dst_stride, dst_frames );
	else hipLaunchKernelGGL( k_copy_rows<false>, grid, dim3( 256 ), 0, s, d_src, src_stride, src_frames, d_dst, dst_stride, dst_frames );
	FLANHIP_CHECK( hipGetLastError() );
	return FLANHIP_OK;
	}

} // extern "C"
